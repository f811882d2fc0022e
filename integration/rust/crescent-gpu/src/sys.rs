//! Raw bindings: one item per declaration of include/crescent_gpu.h that the shim uses.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

pub const CG_FORM_CANONICAL: u32 = 0;
pub const CG_FORM_MONTGOMERY: u32 = 1;
pub const CG_FLAG_H_COEFFICIENT_BASIS: i32 = 1;
pub const CG_FLAG_LATENCY_MODE: i32 = 2;
pub const CG_FLAG_THROUGHPUT_MODE: i32 = 4;
pub const CG_FLAG_SPIN_WAIT: i32 = 8;
pub const CG_FLAG_CONTIGUOUS_H_SHARDS: i32 = 16;
pub const CG_FLAG_H_SCALARS_EXTERNAL: i32 = 32;
pub const CG_FLAG_STAGED_LOAD: i32 = 64;
pub const CG_FLAG_NO_LONE_SLOT: i32 = 128;
pub const CG_FLAG_CHECK_WITNESS: i32 = 256;
pub const CG_FLAG_SCALARS_MONTGOMERY: i32 = 512;
pub const CG_ERR_POLY_DEGREE_TOO_LARGE: c_int = -5;
pub const CG_ERR_MALFORMED_KEY: c_int = -6;
pub const CG_ERR_UNSATISFIED: c_int = -8;
pub const CG_VERIFY_REJECT: u8 = 0;
pub const CG_VERIFY_ACCEPT: u8 = 1;
pub const CG_VERIFY_MALFORMED: u8 = 2;
pub const CG_IO_REVEALED: u8 = 0;
pub const CG_IO_HIDDEN: u8 = 1;
pub const CG_IO_COMMITTED: u8 = 2;
pub const CG_SHOW_MADE: u8 = 1;
pub const CG_SHOW_MALFORMED: u8 = 2;
pub const CG_P256_BAD_SIGNATURE: u8 = 3;
pub const CG_RANGE_N_RAND: usize = 18;
pub const CG_RANGE_N_RESP: usize = 6;

#[repr(C)]
pub struct cg_proving_key {
    pub coord_form: u32,
    pub alpha_g1: *const u8,
    pub beta_g1: *const u8,
    pub delta_g1: *const u8,
    pub beta_g2: *const u8,
    pub delta_g2: *const u8,
    pub a_query: *const u8,
    pub a_len: u64,
    pub b_g1_query: *const u8,
    pub b_g1_len: u64,
    pub b_g2_query: *const u8,
    pub b_g2_len: u64,
    pub h_query: *const u8,
    pub h_len: u64,
    pub l_query: *const u8,
    pub l_len: u64,
}

#[repr(C)]
pub struct cg_csr {
    pub row_ptr: *const u64,
    pub col: *const u32,
    pub coeff: *const u8,
    pub nnz: u64,
}

#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct cg_options {
    pub device: i32,
    pub window_bits: i32,
    pub shard_rank: i32,
    pub shard_count: i32,
    pub proof_slots: i32,
    pub flags: i32,
    pub hw_queues: i32,
    pub shard_span: i32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct cg_timings {
    pub upload_ms: f32,
    pub witness_map_ms: f32,
    pub msm_h_ms: f32,
    pub msm_l_ms: f32,
    pub msm_a_ms: f32,
    pub msm_b1_ms: f32,
    pub msm_b2_ms: f32,
    pub finish_ms: f32,
    pub total_ms: f32,
    pub msm_g1_pairs: u64,
    pub msm_g2_pairs: u64,
    pub accum_g1_ms: f32,
    pub accum_g2_ms: f32,
    pub sort_ms: f32,
    pub reserved_ms: f32,
    pub entries_g1: u64,
    pub entries_g2: u64,
    pub accum_g1_launches: u32,
    pub accum_g2_launches: u32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct cg_ctx_info {
    pub table_bytes: u64,
    pub matrix_bytes: u64,
    pub slot_bytes: u64,
    pub total_bytes: u64,
    pub device_free_bytes: u64,
    pub device_total_bytes: u64,
    pub proof_slots: i32,
    pub window_bits: [i32; 5],
    pub tuned: i32,
    pub retune_skipped_for_memory: i32,
    pub retune_attempts: i32,
    pub shard_rank: i32,
    pub shard_count: i32,
    pub latency_mode: i32,
    pub warmup: i32,
    pub lone_slots: i32,
    pub reserved: [i32; 2],
    pub slot_entry_bytes: u64,
    pub slot_piece_bytes: u64,
    pub slot_bucket_bytes: u64,
    pub slot_transform_bytes: u64,
    pub slot_upload_bytes: u64,
    pub lone_slot_bytes: u64,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct cg_load_timings {
    pub total_ms: f32,
    pub matrices_ms: f32,
    pub domain_ms: f32,
    pub key_copy_ms: f32,
    pub fold_ms: f32,
    pub window_tables_ms: f32,
    pub slots_ms: f32,
    pub final_slots_ms: f32,
    pub background_ms: f32,
    pub swap_wait_ms: f32,
    pub ready_after_ms: f32,
    pub staged: i32,
    pub ready: i32,
    pub windows_from_proof: i32,
    pub warmup_proofs: i32,
    pub background_status: i32,
    pub reserved: [i32; 3],
}

/// `cg_check_witness` / `cg_qap_check_witness`: how many constraints fail, the first of them, its three inner products
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct cg_witness_report {
    pub n_unsatisfied: u64,
    pub first_unsatisfied: u64,
    pub a: [u8; 32],
    pub b: [u8; 32],
    pub c: [u8; 32],
    pub check_ms: f32,
    pub reserved: [i32; 7],
}

/// one range proof of a showing for `cg_verify_showings_batch` and `cg_create_showings_batch`: which committed input, and the
/// (verifying or proving) range key's slot for its bases
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct cg_show_range_link {
    pub committed_index: u32,
    pub slot: u32,
}

/// one range proof per showing, n rows each, in the layouts of `cg_range_verify_proofs_batch`
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct cg_range_rows {
    pub com_f: *const u8,
    pub com_g: *const u8,
    pub com_q: *const u8,
    pub evals: *const u8,
    pub proofs: *const u8,
    pub randomizers: *const u8,
    pub pok_c: *const u8,
    pub pok_s: *const u8,
}

/// one device proof per showing, n rows each (`cg_device_link_verify_batch`); `h_q` may be null with `h_len` 0
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct cg_device_link_rows {
    pub com1: *const u8,
    pub comz: *const u8,
    pub h_q: *const u8,
    pub m: *const u8,
    pub pi0_c: *const u8,
    pub pi0_s: *const u8,
    pub pi1_c: *const u8,
    pub pi1_s: *const u8,
}

/// the scalars one device proof draws: z, t_z, r1, a, b, d, n0, n1, n2 (`cg_device_link_prove_batch`)
pub const CG_DEVICE_LINK_N_RAND: usize = 9;

/// one device proof per showing, n rows each, written by `cg_device_link_prove_batch` in the layouts `cg_device_link_rows` takes
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct cg_device_link_made {
    pub com1: *mut u8,
    pub comz: *mut u8,
    pub m: *mut u8,
    pub pi0_c: *mut u8,
    pub pi0_s: *mut u8,
    pub pi1_c: *mut u8,
    pub pi1_s: *mut u8,
}

/// one range proof per showing, n rows each, in the layouts `cg_range_prove_batch` writes; `challenges` may be null
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct cg_range_made {
    pub com_f: *mut u8,
    pub com_g: *mut u8,
    pub com_q: *mut u8,
    pub evals: *mut u8,
    pub proofs: *mut u8,
    pub pok_c: *mut u8,
    pub pok_s: *mut u8,
    pub challenges: *mut u8,
}

pub enum cg_ctx {}
pub enum cg_partial {}
pub enum cg_msm_ctx {}
pub enum cg_qap_ctx {}
pub enum cg_pvk {}
pub enum cg_range_pk {}
pub enum cg_range_vk {}
pub enum cg_t256_gens {}

extern "C" {
    pub fn cg_init(n_devices: c_int, device_ids: *const c_int) -> c_int;
    pub fn cg_last_error() -> *const c_char;
    pub fn cg_circuit_load(
        out: *mut *mut cg_ctx,
        pk: *const cg_proving_key,
        abc: *const cg_csr,
        num_inputs: u64,
        num_constraints: u64,
        num_variables: u64,
        opt: *const cg_options,
    ) -> c_int;
    pub fn cg_circuit_free(ctx: *mut cg_ctx);
    pub fn cg_prove(
        ctx: *mut cg_ctx,
        full_assignment: *const u8,
        r: *const u8,
        s: *const u8,
        proof_out: *mut u8,
        timings: *mut cg_timings,
    ) -> c_int;
    pub fn cg_host_alloc(bytes: u64) -> *mut c_void;
    pub fn cg_host_free(p: *mut c_void);
    pub fn cg_ctx_get_info(ctx: *mut cg_ctx, out: *mut cg_ctx_info) -> c_int;
    pub fn cg_ctx_get_load_timings(ctx: *mut cg_ctx, out: *mut cg_load_timings) -> c_int;
    pub fn cg_ctx_wait_ready(ctx: *mut cg_ctx, timeout_ms: i32) -> c_int;
    // one proof over several GPUs: this shard's five partial sums; the gathered partials finished into a proof
    pub fn cg_prove_partial(
        ctx: *mut cg_ctx,
        full_assignment: *const c_void,
        assignment_on_device: c_int,
        r: *const u8,
        out_partials: *mut u8,
        timings: *mut cg_timings,
    ) -> c_int;
    pub fn cg_assemble(
        ctx: *mut cg_ctx,
        partials: *const u8,
        n_shards: u32,
        r: *const u8,
        s: *const u8,
        proof_out: *mut u8,
    ) -> c_int;
    // the other arrangement: the witness map once, its values scattered, every shard proves with its slice
    pub fn cg_witness_map_coset(
        ctx: *mut cg_ctx,
        full_assignment: *const c_void,
        assignment_on_device: c_int,
        q_out: *mut c_void,
        q_on_device: c_int,
    ) -> c_int;
    pub fn cg_h_scalars_slice(ctx: *const cg_ctx, shard: u32, offset: *mut u64, count: *mut u64) -> c_int;
    pub fn cg_prove_partial_q(
        ctx: *mut cg_ctx,
        full_assignment: *const c_void,
        assignment_on_device: c_int,
        q_slice: *const c_void,
        q_on_device: c_int,
        r: *const u8,
        out_partials: *mut u8,
        timings: *mut cg_timings,
    ) -> c_int;
    pub fn cg_witness_map(ctx: *mut cg_ctx, full_assignment: *const u8, h_out: *mut u8) -> c_int;
    // cs.is_satisfied() / which_is_unsatisfied() (builder.rs:82-94, prover.rs:197)
    pub fn cg_check_witness(
        ctx: *mut cg_ctx,
        full_assignment: *const c_void,
        assignment_on_device: c_int,
        report: *mut cg_witness_report,
    ) -> c_int;
    // the same in two calls: the l, a, b1, b2 sums start at once, the h share follows the slice
    pub fn cg_prove_partial_q_begin(
        ctx: *mut cg_ctx,
        full_assignment: *const c_void,
        assignment_on_device: c_int,
        r: *const u8,
        out: *mut *mut cg_partial,
    ) -> c_int;
    pub fn cg_partial_witness_map_coset(p: *mut cg_partial, q_out: *mut c_void, q_on_device: c_int) -> c_int;
    pub fn cg_prove_partial_q_finish(
        p: *mut cg_partial,
        q_slice: *const c_void,
        q_on_device: c_int,
        out_partials: *mut u8,
        timings: *mut cg_timings,
    ) -> c_int;
    pub fn cg_prove_partial_q_abort(p: *mut cg_partial);
    // the witness map in two halves: which = 0 the a side, 1 the b side; finish2 multiplies a shard's two slices
    pub fn cg_witness_map_coset_half(
        ctx: *mut cg_ctx,
        full_assignment: *const c_void,
        assignment_on_device: c_int,
        which: c_int,
        out: *mut c_void,
        out_on_device: c_int,
    ) -> c_int;
    pub fn cg_partial_witness_map_coset_half(p: *mut cg_partial, which: c_int, out: *mut c_void, out_on_device: c_int) -> c_int;
    pub fn cg_prove_partial_q_finish2(
        p: *mut cg_partial,
        a_slice: *const c_void,
        b_slice: *const c_void,
        slices_on_device: c_int,
        out_partials: *mut u8,
        timings: *mut cg_timings,
    ) -> c_int;
    pub fn cg_domain_size(ctx: *const cg_ctx) -> u64;
    pub fn cg_qap_load(
        out: *mut *mut cg_qap_ctx,
        abc: *const cg_csr,
        num_inputs: u64,
        num_constraints: u64,
        num_variables: u64,
        device: i32,
    ) -> c_int;
    pub fn cg_qap_load_form(
        out: *mut *mut cg_qap_ctx,
        abc: *const cg_csr,
        num_inputs: u64,
        num_constraints: u64,
        num_variables: u64,
        device: i32,
        scalar_form: u32,
    ) -> c_int;
    pub fn cg_scalars_convert(input: *const u8, in_form: u32, out: *mut u8, out_form: u32, n: u64) -> c_int;
    pub fn cg_qap_witness_map(
        ctx: *mut cg_qap_ctx,
        full_assignment: *const c_void,
        assignment_on_device: c_int,
        h_out: *mut c_void,
        h_on_device: c_int,
    ) -> c_int;
    pub fn cg_qap_check_witness(
        ctx: *mut cg_qap_ctx,
        full_assignment: *const c_void,
        assignment_on_device: c_int,
        report: *mut cg_witness_report,
    ) -> c_int;
    pub fn cg_qap_domain_size(ctx: *const cg_qap_ctx) -> u64;
    pub fn cg_qap_free(ctx: *mut cg_qap_ctx);
    pub fn cg_msm_g1(
        bases: *const u8,
        coord_form: u32,
        n_bases: u64,
        scalars: *const u8,
        n_scalars: u64,
        window_bits: i32,
        out: *mut u8,
    ) -> c_int;
    pub fn cg_msm_g2(
        bases: *const u8,
        coord_form: u32,
        n_bases: u64,
        scalars: *const u8,
        n_scalars: u64,
        window_bits: i32,
        out: *mut u8,
    ) -> c_int;
    pub fn cg_msm_load_g1(
        out: *mut *mut cg_msm_ctx,
        bases: *const u8,
        coord_form: u32,
        n_bases: u64,
        opt: *const cg_options,
    ) -> c_int;
    pub fn cg_msm_run(
        ctx: *mut cg_msm_ctx,
        scalars: *const c_void,
        scalars_on_device: c_int,
        n_scalars: u64,
        out: *mut u8,
        timings: *mut cg_timings,
    ) -> c_int;
    pub fn cg_msm_free(ctx: *mut cg_msm_ctx);
    // verification: a PreparedVerifyingKey resident on a device, proofs and showings in batches
    pub fn cg_pvk_load(out: *mut *mut cg_pvk, pvk_bytes: *const u8, len: u64, device: i32) -> c_int;
    pub fn cg_pvk_num_inputs(k: *const cg_pvk, n: *mut u64) -> c_int;
    pub fn cg_pvk_set_latency_mode(k: *mut cg_pvk, on: i32) -> c_int;
    pub fn cg_pvk_last_kernel_ms(k: *mut cg_pvk, group_ms: *mut f32, pairing_ms: *mut f32) -> c_int;
    pub fn cg_verify_batch(k: *mut cg_pvk, inputs: *const u8, n_inputs: u64, proofs: *const u8, n: u64, verdicts: *mut u8) -> c_int;
    pub fn cg_verify_show_batch(
        k: *mut cg_pvk,
        io_types: *const u8,
        n_io: u64,
        revealed: *const u8,
        rand_proofs: *const u8,
        com_hidden: *const u8,
        committed: *const u8,
        pok_c: *const u8,
        pok_s: *const u8,
        n: u64,
        verdicts: *mut u8,
        k_out: *mut u8,
    ) -> c_int;
    // creating showings: two calls around the host's Merlin transcript
    pub fn cg_show_rand_count(io_types: *const u8, n_io: u64, n_rand: *mut u64) -> c_int;
    pub fn cg_show_commit_batch(
        k: *mut cg_pvk,
        io_types: *const u8,
        n_io: u64,
        proofs: *const u8,
        inputs: *const u8,
        rand: *const u8,
        n: u64,
        rand_proofs: *mut u8,
        com_hidden: *mut u8,
        committed: *mut u8,
        k_out: *mut u8,
        status: *mut u8,
    ) -> c_int;
    pub fn cg_show_respond_batch(
        io_types: *const u8,
        n_io: u64,
        inputs: *const u8,
        rand: *const u8,
        pok_c: *const u8,
        status: *const u8,
        n: u64,
        pok_s: *mut u8,
    ) -> c_int;
    pub fn cg_pvk_free(k: *mut cg_pvk);
    pub fn cg_range_pk_load(
        out: *mut *mut cg_range_pk,
        range_pk_bytes: *const u8,
        len: u64,
        n_bits: u32,
        device: i32,
    ) -> c_int;
    pub fn cg_range_pk_add_bases(k: *mut cg_range_pk, ped_bases: *const u8, slot: *mut u32) -> c_int;
    pub fn cg_range_pk_free(k: *mut cg_range_pk);
    pub fn cg_range_pk_last_kernel_ms(k: *mut cg_range_pk, poly_ms: *mut f32, points_ms: *mut f32) -> c_int;
    pub fn cg_range_commit_batch(
        k: *mut cg_range_pk,
        slot: u32,
        openings: *const u8,
        rand: *const u8,
        n: u64,
        com_f: *mut u8,
        com_g: *mut u8,
        ts_out: *mut u8,
        status: *mut u8,
    ) -> c_int;
    pub fn cg_range_quotient_batch(
        k: *mut cg_range_pk,
        openings: *const u8,
        rand: *const u8,
        c: *const u8,
        n: u64,
        com_q: *mut u8,
        ts_q: *mut u8,
        status: *mut u8,
    ) -> c_int;
    pub fn cg_range_open_batch(
        k: *mut cg_range_pk,
        openings: *const u8,
        rand: *const u8,
        c: *const u8,
        rho: *const u8,
        n: u64,
        evals: *mut u8,
        proofs: *mut u8,
        status: *mut u8,
    ) -> c_int;
    pub fn cg_range_respond_batch(
        openings: *const u8,
        rand: *const u8,
        c_dleq: *const u8,
        status: *const u8,
        n: u64,
        pok_s: *mut u8,
    ) -> c_int;
    pub fn cg_range_vk_load(
        out: *mut *mut cg_range_vk,
        range_vk_bytes: *const u8,
        len: u64,
        n_bits: u32,
        device: i32,
    ) -> c_int;
    pub fn cg_range_vk_add_bases(k: *mut cg_range_vk, ped_bases: *const u8, slot: *mut u32) -> c_int;
    pub fn cg_range_vk_last_kernel_ms(k: *mut cg_range_vk, group_ms: *mut f32, pairing_ms: *mut f32) -> c_int;
    pub fn cg_range_vk_set_latency_mode(k: *mut cg_range_vk, on: i32) -> c_int;
    pub fn cg_range_vk_free(k: *mut cg_range_vk);
    pub fn cg_range_verify_batch(
        k: *mut cg_range_vk,
        slot: u32,
        ped_com: *const u8,
        com_f: *const u8,
        com_g: *const u8,
        com_q: *const u8,
        evals: *const u8,
        proofs: *const u8,
        c: *const u8,
        rho: *const u8,
        randomizers: *const u8,
        pok_c: *const u8,
        pok_s: *const u8,
        n: u64,
        verdicts: *mut u8,
        k_out: *mut u8,
    ) -> c_int;
    pub fn cg_range_prove_batch(
        k: *mut cg_range_pk,
        slot: u32,
        openings: *const u8,
        ped_com: *const u8,
        rand: *const u8,
        n: u64,
        com_f: *mut u8,
        com_g: *mut u8,
        com_q: *mut u8,
        evals: *mut u8,
        proofs: *mut u8,
        pok_c: *mut u8,
        pok_s: *mut u8,
        challenges_out: *mut u8,
        status: *mut u8,
    ) -> c_int;
    pub fn cg_range_verify_proofs_batch(
        k: *mut cg_range_vk,
        slot: u32,
        ped_com: *const u8,
        com_f: *const u8,
        com_g: *const u8,
        com_q: *const u8,
        evals: *const u8,
        proofs: *const u8,
        randomizers: *const u8,
        pok_c: *const u8,
        pok_s: *const u8,
        n: u64,
        verdicts: *mut u8,
    ) -> c_int;
    pub fn cg_dlog_challenge_batch(
        context: *const u8,
        context_len: u64,
        context_stride: u64,
        n_statements: u32,
        n_bases: *const u32,
        bases: *const u8,
        k: *const u8,
        y_head: *const u8,
        y_last: *const u8,
        n: u64,
        c_out: *mut u8,
    ) -> c_int;
    pub fn cg_verify_showings_batch(
        k: *mut cg_pvk,
        rk: *mut cg_range_vk,
        io_types: *const u8,
        n_io: u64,
        context: *const u8,
        context_len: u64,
        context_stride: u64,
        revealed: *const u8,
        rand_proofs: *const u8,
        com_hidden: *const u8,
        committed: *const u8,
        pok_c: *const u8,
        pok_s: *const u8,
        n_ranges: u32,
        links: *const cg_show_range_link,
        shifts: *const u8,
        ranges: *const cg_range_rows,
        n: u64,
        verdicts: *mut u8,
        part_verdicts: *mut u8,
    ) -> c_int;
    pub fn cg_pvk_set_showings_overlap(k: *mut cg_pvk, on: i32) -> c_int;
    pub fn cg_create_showings_batch(
        k: *mut cg_pvk,
        rk: *mut cg_range_pk,
        io_types: *const u8,
        n_io: u64,
        context: *const u8,
        context_len: u64,
        context_stride: u64,
        proofs: *const u8,
        inputs: *const u8,
        rand: *const u8,
        n_ranges: u32,
        links: *const cg_show_range_link,
        shifts: *const u8,
        range_rand: *const u8,
        n: u64,
        rand_proofs: *mut u8,
        com_hidden: *mut u8,
        committed: *mut u8,
        pok_c: *mut u8,
        pok_s: *mut u8,
        ranges: *const cg_range_made,
        status: *mut u8,
        part_status: *mut u8,
    ) -> c_int;
    pub fn cg_show_shift_batch(
        k: *mut cg_pvk,
        input_index: u32,
        openings: *const u8,
        commitments: *const u8,
        shifts: *const u8,
        n: u64,
        openings_out: *mut u8,
        ped_com_out: *mut u8,
        status: *mut u8,
    ) -> c_int;
    pub fn cg_device_link_verify_batch(
        k: *mut cg_pvk,
        io_types: *const u8,
        n_io: u64,
        pos0: u32,
        pos1: u32,
        committed: *const u8,
        rows: *const cg_device_link_rows,
        h_len: u32,
        n: u64,
        verdicts: *mut u8,
        part_verdicts: *mut u8,
        e_out: *mut u8,
    ) -> c_int;
    pub fn cg_device_link_last_kernel_ms(k: *mut cg_pvk, ms: *mut f32) -> c_int;
    pub fn cg_device_link_prove_batch(
        k: *mut cg_pvk,
        io_types: *const u8,
        n_io: u64,
        pos0: u32,
        pos1: u32,
        committed: *const u8,
        openings: *const u8,
        rand: *const u8,
        h_q: *const u8,
        h_len: u32,
        n: u64,
        out: *const cg_device_link_made,
        e_out: *mut u8,
        status: *mut u8,
    ) -> c_int;
    pub fn cg_device_link_prove_last_kernel_ms(k: *mut cg_pvk, ms: *mut f32) -> c_int;
    pub fn cg_poseidon_p256_permute_batch(k: *mut cg_pvk, states: *const u8, n: u64, out: *mut u8, status: *mut u8) -> c_int;
    pub fn cg_hq_batch(k: *mut cg_pvk, q: *const u8, n: u64, h_q_out: *mut u8, status: *mut u8) -> c_int;
    pub fn cg_device_link_prove_hq_batch(
        k: *mut cg_pvk,
        io_types: *const u8,
        n_io: u64,
        pos0: u32,
        pos1: u32,
        committed: *const u8,
        openings: *const u8,
        rand: *const u8,
        n: u64,
        out: *const cg_device_link_made,
        e_out: *mut u8,
        status: *mut u8,
        h_q_out: *mut u8,
    ) -> c_int;
    pub fn cg_hq_last_kernel_ms(k: *mut cg_pvk, ms: *mut f32, uploads: *mut u32) -> c_int;
    pub fn cg_p256_tu_batch(k: *mut cg_pvk, r_xy: *const u8, digest: *const u8, n: u64, t_xy: *mut u8, u_xy: *mut u8, status: *mut u8) -> c_int;
    pub fn cg_p256_rtu_batch(
        k: *mut cg_pvk,
        q_xy: *const u8,
        sig: *const u8,
        digest: *const u8,
        n: u64,
        r_xy: *mut u8,
        t_xy: *mut u8,
        u_xy: *mut u8,
        status: *mut u8,
    ) -> c_int;
    pub fn cg_p256_last_kernel_ms(k: *mut cg_pvk, ms: *mut f32, uploads: *mut u32) -> c_int;
    pub fn cg_t256_gens_load(g_xy: *const u8, n_gens: u64, h_xy: *const u8, out: *mut *mut cg_t256_gens) -> c_int;
    pub fn cg_t256_gens_free(g: *mut cg_t256_gens);
    pub fn cg_t256_gens_info(g: *const cg_t256_gens, n_gens: *mut u64, table_bytes: *mut u64) -> c_int;
    pub fn cg_t256_commit_rows_batch(g: *mut cg_t256_gens, scalars: *const u8, blinds: *const u8, n_rows: u64, out33: *mut u8, status: *mut u8) -> c_int;
    pub fn cg_hyrax_commit_batch(
        g: *mut cg_t256_gens,
        num_vars: u32,
        vars: *const u8,
        blinds: *const u8,
        n: u64,
        out33: *mut u8,
        status: *mut u8,
    ) -> c_int;
    pub fn cg_t256_commit_last_kernel_ms(g: *mut cg_t256_gens, ms: *mut f32, lanes_per_row: *mut u32) -> c_int;
    pub fn cg_revealed_digest_batch(data: *const u8, offsets: *const u64, n_items: u64, out: *mut u8) -> c_int;
}
