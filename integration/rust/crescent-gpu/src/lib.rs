//! Safe wrapper: a Groth16 circuit resident on one MI355X, proving through `cg_prove`.
//!
//! `GpuCircuit::create_proof` has the semantics of
//! `Groth16::<Bn254, LibsnarkReduction>::create_proof_with_reduction_and_matrices`
//! (forks/groth16/src/prover.rs:26-51): same operands, same `Proof`, byte for byte.
pub mod sys;

use ark_bn254::{Bn254, Fq, Fq2, Fr, G1Affine, G2Affine};
use ark_ff::{BigInt, BigInteger, PrimeField};
use ark_groth16::r1cs_to_qap::{LibsnarkReduction, R1CSToQAP};
use ark_groth16::{Proof, ProvingKey};
use ark_poly::EvaluationDomain;
use ark_relations::r1cs::{ConstraintMatrices, ConstraintSystemRef, SynthesisError};
use ark_serialize::{CanonicalDeserialize, CanonicalSerialize};
use std::collections::HashMap;
use std::ffi::CStr;
use std::sync::{Arc, Mutex, OnceLock};

// `Affine { x, y, infinity }` is repr(Rust): coordinates are packed into byte arrays, struct pointers never
// cross the boundary.  The Montgomery limbs are copied as they are (`Fp.0` is the BigInt of x·2^256 mod p, the
// form forks/circom-compat/src/zkey.rs:397-402 pins), so no field arithmetic happens on this side.
fn put_fq(out: &mut [u8], x: &Fq) {
    for (k, limb) in x.0 .0.iter().enumerate() {
        out[k * 8..k * 8 + 8].copy_from_slice(&limb.to_le_bytes());
    }
}
// The same for scalars: every context this crate loads carries `CG_FLAG_SCALARS_MONTGOMERY` (and `GpuReduction`'s handle
// `CG_FORM_MONTGOMERY`), so an assignment crosses as the limbs of `Fr.0` - a copy, where `into_bigint()` was a Montgomery
// reduction per element on one host thread - and the GPU converts.  32 bytes per element is what the library reads:
const _: () = assert!(std::mem::size_of::<Fr>() == 32);
fn put_fr(out: &mut [u8], x: &Fr) {
    for (k, limb) in x.0 .0.iter().enumerate() {
        out[k * 8..k * 8 + 8].copy_from_slice(&limb.to_le_bytes());
    }
}
/// An assignment as the library takes it on this crate's contexts: `Fr.0`, limb by limb (no arithmetic).
fn montgomery_bytes(xs: &[Fr]) -> Vec<u8> {
    let mut out = vec![0u8; xs.len() * 32];
    for (i, x) in xs.iter().enumerate() {
        put_fr(&mut out[i * 32..i * 32 + 32], x);
    }
    out
}
fn put_fq2(out: &mut [u8], x: &Fq2) {
    put_fq(&mut out[..32], &x.c0);
    put_fq(&mut out[32..64], &x.c1);
}
fn pack_g1(v: &[G1Affine]) -> Vec<u8> {
    let mut out = vec![0u8; v.len() * 64];
    for (i, p) in v.iter().enumerate() {
        if p.infinity {
            continue; // identity = 64 zero bytes
        }
        put_fq(&mut out[i * 64..i * 64 + 32], &p.x);
        put_fq(&mut out[i * 64 + 32..i * 64 + 64], &p.y);
    }
    out
}
fn pack_g2(v: &[G2Affine]) -> Vec<u8> {
    let mut out = vec![0u8; v.len() * 128];
    for (i, p) in v.iter().enumerate() {
        if p.infinity {
            continue; // identity = 128 zero bytes
        }
        put_fq2(&mut out[i * 128..i * 128 + 64], &p.x); // x.c0 ‖ x.c1
        put_fq2(&mut out[i * 128 + 64..i * 128 + 128], &p.y); // y.c0 ‖ y.c1
    }
    out
}

struct Csr {
    row_ptr: Vec<u64>,
    col: Vec<u32>,
    coeff: Vec<u8>,
}
fn to_csr<F: PrimeField>(rows: &[Vec<(F, usize)>]) -> Csr {
    let mut m = Csr { row_ptr: vec![0u64], col: Vec::new(), coeff: Vec::new() };
    for row in rows {
        for (c, j) in row {
            m.col.push(*j as u32);
            m.coeff.extend_from_slice(&c.into_bigint().to_bytes_le()); // canonical, 32 bytes
        }
        m.row_ptr.push(m.col.len() as u64);
    }
    m
}
impl Csr {
    fn view(&self) -> sys::cg_csr {
        sys::cg_csr { row_ptr: self.row_ptr.as_ptr(), col: self.col.as_ptr(), coeff: self.coeff.as_ptr(), nnz: self.col.len() as u64 }
    }
}

fn last_error() -> String {
    unsafe { CStr::from_ptr(sys::cg_last_error()).to_string_lossy().into_owned() }
}
fn map_err(rc: i32) -> SynthesisError {
    eprintln!("crescent-gpu: {} (code {})", last_error(), rc);
    match rc {
        sys::CG_ERR_POLY_DEGREE_TOO_LARGE => SynthesisError::PolynomialDegreeTooLarge, // r1cs_to_qap.rs:156-157
        sys::CG_ERR_MALFORMED_KEY => SynthesisError::MalformedVerifyingKey,
        sys::CG_ERR_UNSATISFIED => SynthesisError::Unsatisfiable, // a context loaded with CG_FLAG_CHECK_WITNESS
        _ => SynthesisError::AssignmentMissing, // no twin in SynthesisError; the message is on stderr
    }
}

/// Page-locked host bytes from `cg_host_alloc`, freed with `cg_host_free`.
struct PinnedBytes {
    ptr: *mut u8,
    len: usize,
}
impl PinnedBytes {
    /// None when the page-lock fails (the caller then falls back to pageable memory, which `cg_prove` also takes)
    fn new(len: usize) -> Option<Self> {
        let p = unsafe { sys::cg_host_alloc(len as u64) } as *mut u8;
        if p.is_null() {
            eprintln!("crescent-gpu: page-locked witness buffer unavailable ({}): using pageable memory", last_error());
            return None;
        }
        Some(PinnedBytes { ptr: p, len })
    }
    #[allow(clippy::mut_from_ref)]
    fn slice_mut(&self) -> &mut [u8] {
        unsafe { std::slice::from_raw_parts_mut(self.ptr, self.len) }
    }
}
impl Drop for PinnedBytes {
    fn drop(&mut self) {
        unsafe { sys::cg_host_free(self.ptr as *mut std::os::raw::c_void) }
    }
}

// PinnedBytes is only ever touched by the thread that took it out of the pool
unsafe impl Send for PinnedBytes {}

pub struct GpuCircuit {
    ctx: *mut sys::cg_ctx,
    num_variables: usize,
    /// Page-locked witness buffers, kept for the life of the circuit: `hipHostMalloc` page-locks 48 MB at full size (a few
    /// milliseconds) and `hipHostFree` synchronises the WHOLE device, so allocating and freeing one per proof would stall
    /// every finishing caller behind every proof in flight.  A proof takes a buffer out and puts it back; at most
    /// `pool_max` (= proof_slots + 2, the upload buffers the context holds) are retained, all freed in `Drop`.
    pool: Mutex<Vec<PinnedBytes>>,
    pool_max: usize,
}
// calls on one context are multiplexed over its proof slots inside the library
unsafe impl Send for GpuCircuit {}
unsafe impl Sync for GpuCircuit {}

impl GpuCircuit {
    /// One-time: pack the key and the matrices and copy them to the GPU (`cg_circuit_load`).
    /// `proof_slots` = proofs that may be in flight on this circuit at once (one per calling thread).
    /// The load is STAGED (`CG_FLAG_STAGED_LOAD`): it returns as soon as the circuit can prove and the library finishes its
    /// tables behind the first proofs - what `create_client_state` (creds/src/lib.rs:255-301), which loads and proves once,
    /// wants.  A host that is about to stream proofs may call `wait_ready` first.
    pub fn load(pk: &ProvingKey<Bn254>, m: &ConstraintMatrices<Fr>, device: i32, proof_slots: i32) -> Result<Self, SynthesisError> {
        Self::load_with_flags(pk, m, device, proof_slots, sys::CG_FLAG_STAGED_LOAD)
    }

    /// `load` with the context's flags spelt out (`sys::CG_FLAG_*`; 0 = the synchronous load).
    pub fn load_with_flags(pk: &ProvingKey<Bn254>, m: &ConstraintMatrices<Fr>, device: i32, proof_slots: i32, flags: i32)
                           -> Result<Self, SynthesisError> {
        Self::load_opt(pk, m, sys::cg_options { device, proof_slots, flags, ..Default::default() })
    }

    /// One shard of a proof split over `shard_count` GPUs (`cg_options.shard_rank / shard_count`): the context
    /// owns its ranges of the five queries and answers `prove_partial` (or, loaded with `CG_FLAG_H_SCALARS_EXTERNAL`,
    /// `prove_partial_q` only).  `assemble` on any shard finishes the gathered partial sums into the proof.
    pub fn load_shard(pk: &ProvingKey<Bn254>, m: &ConstraintMatrices<Fr>, device: i32, proof_slots: i32, shard_rank: i32,
                      shard_count: i32, flags: i32) -> Result<Self, SynthesisError> {
        Self::load_opt(pk, m, sys::cg_options { device, proof_slots, shard_rank, shard_count, flags, ..Default::default() })
    }

    /// `load_shard` with an UNEQUAL share (`cg_options.shard_span`): the shard owns `[n·lo/10000, n·hi/10000)` of every query.
    /// The spans of a proof's shards must tile `[0, 10000]`; the ranks that also compute (half of) the witness map take the
    /// smaller ones.
    pub fn load_shard_span(pk: &ProvingKey<Bn254>, m: &ConstraintMatrices<Fr>, device: i32, proof_slots: i32, shard_rank: i32,
                           shard_count: i32, span: (u16, u16), flags: i32) -> Result<Self, SynthesisError> {
        let shard_span = span.0 as i32 | ((span.1 as i32) << 16);
        Self::load_opt(pk, m, sys::cg_options { device, proof_slots, shard_rank, shard_count, flags, shard_span, ..Default::default() })
    }

    fn load_opt(pk: &ProvingKey<Bn254>, m: &ConstraintMatrices<Fr>, mut opt: sys::cg_options) -> Result<Self, SynthesisError> {
        // every wrapper below hands the library `Fr.0` as it lies in memory (put_fr): the context converts on the GPU
        opt.flags |= sys::CG_FLAG_SCALARS_MONTGOMERY;
        let proof_slots = opt.proof_slots;
        let rc = unsafe { sys::cg_init(0, std::ptr::null()) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        let (alpha, beta1, delta1) = (pack_g1(&[pk.vk.alpha_g1]), pack_g1(&[pk.beta_g1]), pack_g1(&[pk.delta_g1]));
        let (beta2, delta2) = (pack_g2(&[pk.vk.beta_g2]), pack_g2(&[pk.vk.delta_g2]));
        let (a, b1, h, l) = (pack_g1(&pk.a_query), pack_g1(&pk.b_g1_query), pack_g1(&pk.h_query), pack_g1(&pk.l_query));
        let b2 = pack_g2(&pk.b_g2_query);
        let view = sys::cg_proving_key {
            coord_form: sys::CG_FORM_MONTGOMERY,
            alpha_g1: alpha.as_ptr(),
            beta_g1: beta1.as_ptr(),
            delta_g1: delta1.as_ptr(),
            beta_g2: beta2.as_ptr(),
            delta_g2: delta2.as_ptr(),
            a_query: a.as_ptr(),
            a_len: pk.a_query.len() as u64,
            b_g1_query: b1.as_ptr(),
            b_g1_len: pk.b_g1_query.len() as u64,
            b_g2_query: b2.as_ptr(),
            b_g2_len: pk.b_g2_query.len() as u64,
            h_query: h.as_ptr(),
            h_len: pk.h_query.len() as u64,
            l_query: l.as_ptr(),
            l_len: pk.l_query.len() as u64,
        };
        let (ca, cb, cc) = (to_csr(&m.a), to_csr(&m.b), to_csr(&m.c));
        let abc = [ca.view(), cb.view(), cc.view()];
        let num_variables = m.num_instance_variables + m.num_witness_variables;
        let mut ctx: *mut sys::cg_ctx = std::ptr::null_mut();
        let rc = unsafe {
            sys::cg_circuit_load(&mut ctx, &view, abc.as_ptr(), m.num_instance_variables as u64, m.num_constraints as u64,
                                 num_variables as u64, &opt)
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(GpuCircuit { ctx, num_variables, pool: Mutex::new(Vec::new()), pool_max: proof_slots.max(1) as usize + 2 })
    }

    /// forks/groth16/src/prover.rs:26-51 with the key and the matrices already resident on the GPU.
    /// `full_assignment` = instance assignment ‖ witness assignment (element 0 is the constant one).
    pub fn create_proof(&self, r: Fr, s: Fr, full_assignment: &[Fr]) -> Result<Proof<Bn254>, SynthesisError> {
        if full_assignment.len() != self.num_variables {
            return Err(SynthesisError::AssignmentMissing);
        }
        // the limbs of `Fr.0` are copied straight into page-locked memory from the circuit's pool: cg_prove's upload is
        // then one asynchronous DMA at PCIe speed that overlaps the other proofs in flight.  Should page-locking fail
        // (locked-memory limit of the host), a pageable Vec does the same job a little slower - never an error.
        let len = full_assignment.len() * 32;
        let pinned = self.pool.lock().unwrap().pop().or_else(|| PinnedBytes::new(len));
        let mut pageable: Vec<u8> = Vec::new();
        let buf: &mut [u8] = match &pinned {
            Some(p) => p.slice_mut(),
            None => {
                pageable.resize(len, 0);
                &mut pageable[..]
            }
        };
        for (i, x) in full_assignment.iter().enumerate() {
            put_fr(&mut buf[i * 32..i * 32 + 32], x); // CG_FLAG_SCALARS_MONTGOMERY: the `into_bigint` of prover.rs:64,71,86 runs on the GPU
        }
        let (rb, sb) = (r.into_bigint().to_bytes_le(), s.into_bigint().to_bytes_le());
        let mut out = [0u8; 256];
        // the phases the reference prints under its `print-trace` feature (forks/groth16/Cargo.toml:48; start_timer! /
        // end_timer! at prover.rs:35-36,62,93,103,115,123), with the GPU's own times: cg_timings mirrors them 1:1
        let mut tm = sys::cg_timings::default();
        let tm_ptr: *mut sys::cg_timings = if cfg!(feature = "print-trace") { &mut tm } else { std::ptr::null_mut() };
        let rc = unsafe { sys::cg_prove(self.ctx, buf.as_ptr(), rb.as_ptr(), sb.as_ptr(), out.as_mut_ptr(), tm_ptr) };
        #[cfg(feature = "print-trace")]
        if rc == 0 {
            print_trace(&tm);
        }
        if let Some(p) = pinned {
            let mut pool = self.pool.lock().unwrap();
            if pool.len() < self.pool_max {
                pool.push(p); // kept for the next proof; a surplus buffer (more callers than slots + 2) is freed here
            }
        }
        if rc != 0 {
            return Err(map_err(rc));
        }
        // a ‖ b ‖ c, ark-serialize uncompressed (data_structures.rs:7-14)
        Proof::deserialize_uncompressed_unchecked(&out[..]).map_err(|_| SynthesisError::MalformedVerifyingKey)
    }
}

/// The reference's `print-trace` output for one proof, phase names as prover.rs spells them, times from cg_timings (the
/// five MSMs overlap on the GPU, so the phases do not add up to the total the way the CPU prover's do).
#[cfg(feature = "print-trace")]
fn print_trace(tm: &sys::cg_timings) {
    let line = |depth: usize, name: &str, ms: f32| println!("{}End:     {} {:.3}ms", "··".repeat(depth), name, ms);
    println!("Start:   Groth16::Prover");                                                  // prover.rs:35
    line(1, "R1CS to QAP witness map", tm.witness_map_ms);                                 // :36
    line(1, "Compute C", tm.msm_h_ms.max(tm.msm_l_ms));                                    // :62  (h_query and l_query MSMs)
    line(1, "Compute A", tm.msm_a_ms);                                                     // :93
    line(1, "Compute B in G1", tm.msm_b1_ms);                                              // :103 (0 when r = 0: skipped, :102-112)
    line(1, "Compute B in G2", tm.msm_b2_ms);                                              // :115
    line(1, "Finish C", tm.finish_ms);                                                     // :123
    line(1, "(upload of the assignment)", tm.upload_ms);
    line(0, "Groth16::Prover", tm.total_ms);                                               // :48
}

/// Canonical bytes (`into_bigint`): what stays canonical on every context - r, s, the showings' small vectors (pok_*, inputs, rand).
fn canonical_bytes(xs: &[Fr]) -> Vec<u8> {
    let mut out = vec![0u8; xs.len() * 32];
    for (i, x) in xs.iter().enumerate() {
        out[i * 32..i * 32 + 32].copy_from_slice(&x.into_bigint().to_bytes_le());
    }
    out
}

/// One proof over several GPUs, on contexts made by `GpuCircuit::load_shard`.  The 384-byte partial records
/// are what the host gathers (one per shard); nothing else crosses between the shards.
impl GpuCircuit {
    /// This shard's five partial sums h ‖ l ‖ a ‖ b1 ‖ b2 (`cg_prove_partial`; prover.rs:66,74,266 over the shard's ranges).
    pub fn prove_partial(&self, r: Fr, full_assignment: &[Fr]) -> Result<[u8; 384], SynthesisError> {
        if full_assignment.len() != self.num_variables {
            return Err(SynthesisError::AssignmentMissing);
        }
        let (w, rb) = (montgomery_bytes(full_assignment), r.into_bigint().to_bytes_le());
        let mut out = [0u8; 384];
        let rc = unsafe { sys::cg_prove_partial(self.ctx, w.as_ptr() as *const _, 0, rb.as_ptr(), out.as_mut_ptr(), std::ptr::null_mut()) };
        if rc != 0 { Err(map_err(rc)) } else { Ok(out) }
    }

    /// The gathered partial sums of all shards -> the proof (`cg_assemble`; prover.rs:76-135).
    pub fn assemble(&self, partials: &[[u8; 384]], r: Fr, s: Fr) -> Result<Proof<Bn254>, SynthesisError> {
        let flat: Vec<u8> = partials.iter().flat_map(|p| p.iter().copied()).collect();
        let (rb, sb) = (r.into_bigint().to_bytes_le(), s.into_bigint().to_bytes_le());
        let mut out = [0u8; 256];
        let rc = unsafe { sys::cg_assemble(self.ctx, flat.as_ptr(), partials.len() as u32, rb.as_ptr(), sb.as_ptr(), out.as_mut_ptr()) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Proof::deserialize_uncompressed_unchecked(&out[..]).map_err(|_| SynthesisError::MalformedVerifyingKey)
    }

    /// SURVEY 8e's other arrangement, step 1 (`cg_witness_map_coset`): the witness map ONCE, on a context loaded without
    /// `CG_FLAG_H_SCALARS_EXTERNAL`; all `domain_size` coset values as 32-byte canonical scalars, laid out shard-major so
    /// that shard p's share is the contiguous range `h_scalars_slice(p)` - what a scatter sends.
    pub fn witness_map_coset(&self, full_assignment: &[Fr]) -> Result<Vec<u8>, SynthesisError> {
        if full_assignment.len() != self.num_variables {
            return Err(SynthesisError::AssignmentMissing);
        }
        let w = montgomery_bytes(full_assignment);
        let mut q = vec![0u8; unsafe { sys::cg_domain_size(self.ctx) } as usize * 32];
        let rc = unsafe { sys::cg_witness_map_coset(self.ctx, w.as_ptr() as *const _, 0, q.as_mut_ptr() as *mut _, 0) };
        if rc != 0 { Err(map_err(rc)) } else { Ok(q) }
    }

    /// (offset, count), in scalars, of shard `shard`'s share of `witness_map_coset`'s output (`cg_h_scalars_slice`).
    pub fn h_scalars_slice(&self, shard: u32) -> Result<(u64, u64), SynthesisError> {
        let (mut off, mut cnt) = (0u64, 0u64);
        let rc = unsafe { sys::cg_h_scalars_slice(self.ctx, shard, &mut off, &mut cnt) };
        if rc != 0 { Err(map_err(rc)) } else { Ok((off, cnt)) }
    }

    /// Step 2 (`cg_prove_partial_q`): this shard's partial sums with its slice of the coset values supplied; the only way a
    /// context loaded with `CG_FLAG_H_SCALARS_EXTERNAL` proves.
    pub fn prove_partial_q(&self, r: Fr, full_assignment: &[Fr], q_slice: &[u8]) -> Result<[u8; 384], SynthesisError> {
        if full_assignment.len() != self.num_variables {
            return Err(SynthesisError::AssignmentMissing);
        }
        let (w, rb) = (montgomery_bytes(full_assignment), r.into_bigint().to_bytes_le());
        let mut out = [0u8; 384];
        let rc = unsafe {
            sys::cg_prove_partial_q(self.ctx, w.as_ptr() as *const _, 0, q_slice.as_ptr() as *const _, 0, rb.as_ptr(), out.as_mut_ptr(),
                                    std::ptr::null_mut())
        };
        if rc != 0 { Err(map_err(rc)) } else { Ok(out) }
    }
}

/// A sharded proof between `cg_prove_partial_q_begin` and `_finish` / `_finish2`: the shard's l, a, b1, b2 partial sums are
/// queued and running; the h share follows once the slice (or the two halves' slices) has arrived.  Holds one of the circuit's
/// proof slots; dropped unfinished, it is aborted (`cg_prove_partial_q_abort`).
pub struct OpenProof<'a> {
    p: *mut sys::cg_partial,
    circuit: &'a GpuCircuit,
}

impl GpuCircuit {
    /// `cg_prove_partial_q_begin`: open a sharded proof; returns while the assignment-driven sums run.
    pub fn prove_partial_q_begin(&self, r: Fr, full_assignment: &[Fr]) -> Result<OpenProof<'_>, SynthesisError> {
        if full_assignment.len() != self.num_variables {
            return Err(SynthesisError::AssignmentMissing);
        }
        let (w, rb) = (montgomery_bytes(full_assignment), r.into_bigint().to_bytes_le());
        let mut p: *mut sys::cg_partial = std::ptr::null_mut();
        // (the library has copied the assignment to the GPU before it returns: `w` may go)
        let rc = unsafe { sys::cg_prove_partial_q_begin(self.ctx, w.as_ptr() as *const _, 0, rb.as_ptr(), &mut p) };
        if rc != 0 { Err(map_err(rc)) } else { Ok(OpenProof { p, circuit: self }) }
    }
}

impl<'a> OpenProof<'a> {
    /// One side of the coset values for this proof's assignment (`cg_partial_witness_map_coset_half`): `which` = 0 the a side,
    /// 1 the b side; `domain_size` plain canonical scalars, laid out like `witness_map_coset`'s output.
    pub fn witness_map_coset_half(&self, which: i32) -> Result<Vec<u8>, SynthesisError> {
        let mut q = vec![0u8; unsafe { sys::cg_domain_size(self.circuit.ctx) } as usize * 32];
        let rc = unsafe { sys::cg_partial_witness_map_coset_half(self.p, which, q.as_mut_ptr() as *mut _, 0) };
        if rc != 0 { Err(map_err(rc)) } else { Ok(q) }
    }

    /// `cg_prove_partial_q_finish`: the h share with this shard's slice of the coset values -> the 384-byte record.
    pub fn finish(mut self, q_slice: &[u8]) -> Result<[u8; 384], SynthesisError> {
        let mut out = [0u8; 384];
        let p = std::mem::replace(&mut self.p, std::ptr::null_mut());      // the call consumes the handle, success or not
        let rc = unsafe { sys::cg_prove_partial_q_finish(p, q_slice.as_ptr() as *const _, 0, out.as_mut_ptr(), std::ptr::null_mut()) };
        if rc != 0 { Err(map_err(rc)) } else { Ok(out) }
    }

    /// `cg_prove_partial_q_finish2`: the same from the shard's slices of BOTH sides; their products are formed on the GPU.
    pub fn finish2(mut self, a_slice: &[u8], b_slice: &[u8]) -> Result<[u8; 384], SynthesisError> {
        let mut out = [0u8; 384];
        let p = std::mem::replace(&mut self.p, std::ptr::null_mut());
        let rc = unsafe {
            sys::cg_prove_partial_q_finish2(p, a_slice.as_ptr() as *const _, b_slice.as_ptr() as *const _, 0, out.as_mut_ptr(), std::ptr::null_mut())
        };
        if rc != 0 { Err(map_err(rc)) } else { Ok(out) }
    }
}

impl<'a> Drop for OpenProof<'a> {
    fn drop(&mut self) {
        if !self.p.is_null() {
            unsafe { sys::cg_prove_partial_q_abort(self.p) }
        }
    }
}

impl GpuCircuit {
    /// Blocks until a staged load's final arrangement is in force (`cg_ctx_wait_ready`); `Ok(false)` = the time ran out
    /// first.  `timeout_ms < 0` waits without limit.  Proofs made before that are the same bytes, only slower.
    pub fn wait_ready(&self, timeout_ms: i32) -> Result<bool, SynthesisError> {
        match unsafe { sys::cg_ctx_wait_ready(self.ctx, timeout_ms) } {
            0 => Ok(true),
            1 => Ok(false),
            rc => Err(map_err(rc)),
        }
    }

    /// Where the load's time went (`cg_ctx_get_load_timings`): the counterpart of the reference's "Reading ProverParams" /
    /// "Reading R1CS" timers (creds/src/lib.rs:257,266).
    pub fn load_timings(&self) -> Result<sys::cg_load_timings, SynthesisError> {
        let mut t = sys::cg_load_timings::default();
        let rc = unsafe { sys::cg_ctx_get_load_timings(self.ctx, &mut t) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(t)
    }

    /// `cs.is_satisfied()` / `cs.which_is_unsatisfied()` (forks/circom-compat/src/circom/builder.rs:82-94; the debug assertion
    /// of forks/groth16/src/prover.rs:197) on the GPU (`cg_check_witness`): `Ok(None)` = every constraint holds, `Ok(Some(report))`
    /// = `report.first_unsatisfied` is the first of `report.n_unsatisfied` failing constraints and `a`, `b`, `c` its three inner
    /// products.  A context loaded with `sys::CG_FLAG_CHECK_WITNESS` runs the same check inside every `create_proof`.
    pub fn check_witness(&self, full_assignment: &[Fr]) -> Result<Option<sys::cg_witness_report>, SynthesisError> {
        if full_assignment.len() != self.num_variables {
            return Err(SynthesisError::AssignmentMissing);
        }
        let w = montgomery_bytes(full_assignment);
        let mut rep = sys::cg_witness_report::default();
        match unsafe { sys::cg_check_witness(self.ctx, w.as_ptr() as *const _, 0, &mut rep) } {
            0 => Ok(None),
            sys::CG_ERR_UNSATISFIED => Ok(Some(rep)),
            rc => Err(map_err(rc)),
        }
    }

    /// What the circuit occupies on the GPU and how its MSMs are configured (`cg_ctx_get_info`).
    pub fn info(&self) -> Result<sys::cg_ctx_info, SynthesisError> {
        let mut i = sys::cg_ctx_info::default();
        let rc = unsafe { sys::cg_ctx_get_info(self.ctx, &mut i) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(i)
    }
}

impl Drop for GpuCircuit {
    fn drop(&mut self) {
        unsafe { sys::cg_circuit_free(self.ctx) } // waits for calls still inside the context
        self.pool.lock().unwrap().clear(); // cg_host_free: the one place the pinned buffers are released
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The reference's own plug point: `Groth16<E, QAP: R1CSToQAP = LibsnarkReduction>` (forks/groth16/src/lib.rs:55-57).
// `Groth16::<Bn254, GpuReduction>::prove(..)` keeps the whole of prover.rs - synthesis, arkworks' MSMs - and moves the
// witness map (three sparse products, seven transforms; r1cs_to_qap.rs:150-213) to the GPU through cg_qap_*.  It is the
// smaller of the two integrations (the other being `GpuCircuit`, which also takes the five MSMs); both give the same bytes.
// ---------------------------------------------------------------------------------------------------------------
struct QapHandle(*mut sys::cg_qap_ctx);
unsafe impl Send for QapHandle {}
unsafe impl Sync for QapHandle {} // calls on one handle serialise inside the library
impl Drop for QapHandle {
    fn drop(&mut self) {
        unsafe { sys::cg_qap_free(self.0) }
    }
}

/// Matrices are constants of a credential type but arrive by reference on every call (r1cs_to_qap.rs:150-155), so the
/// resident copy is looked up by a digest of their WHOLE content: the shape, the non-zero counts and two independent
/// 64-bit FNV-1a passes over every term (all four limbs of every coefficient, every column index, every row boundary).
/// One pass over the 17 M terms of a full-size circuit costs a few tens of milliseconds - the reference's own call spends
/// seconds in the transforms it replaces.  (Round 2 sampled every 1024th term: two circuits of the same shape that
/// differed in an unsampled coefficient would have shared a resident copy and produced a wrong h without an error.)
fn fingerprint<F: PrimeField>(m: &ConstraintMatrices<F>) -> [u64; 8] {
    const P: u64 = 0x0000_0100_0000_01b3; // FNV-1a 64 prime
    let (mut h1, mut h2) = (0xcbf2_9ce4_8422_2325u64, 0x8422_2325_cbf2_9ce4u64);
    let mut eat = |v: u64| {
        h1 = (h1 ^ v).wrapping_mul(P);
        h2 = (h2 ^ v.rotate_left(29) ^ 0x9e37_79b9_7f4a_7c15).wrapping_mul(P).rotate_left(5);
    };
    for mat in [&m.a, &m.b, &m.c] {
        for row in mat.iter() {
            eat(0xffff_ffff_0000_0000 | row.len() as u64); // row boundary
            for (c, j) in row {
                for limb in c.into_bigint().as_ref() {
                    eat(*limb);
                }
                eat(*j as u64);
            }
        }
        eat(0x5a5a_5a5a_5a5a_5a5a); // matrix boundary
    }
    [
        m.num_instance_variables as u64, m.num_witness_variables as u64, m.num_constraints as u64,
        m.a_num_non_zero as u64, m.b_num_non_zero as u64, m.c_num_non_zero as u64, h1, h2,
    ]
}

/// At most this many circuits keep a device copy of their matrices; the least recently used one is dropped first.  A
/// dropped entry's `cg_qap_free` runs when its last `Arc` holder (a call still in flight) lets go - never under a caller.
const QAP_CACHE_MAX: usize = 4;
struct QapCache {
    tick: u64,
    entries: HashMap<[u64; 8], (u64, Arc<QapHandle>)>, // key -> (last use, handle)
}
fn qap_for<F: PrimeField>(m: &ConstraintMatrices<F>) -> Result<Arc<QapHandle>, SynthesisError> {
    static CACHE: OnceLock<Mutex<QapCache>> = OnceLock::new();
    let key = fingerprint(m);
    let mut cache = CACHE.get_or_init(|| Mutex::new(QapCache { tick: 0, entries: HashMap::new() })).lock().unwrap();
    cache.tick += 1;
    let now = cache.tick;
    if let Some(e) = cache.entries.get_mut(&key) {
        e.0 = now;
        return Ok(e.1.clone());
    }
    let rc = unsafe { sys::cg_init(0, std::ptr::null()) };
    if rc != 0 {
        return Err(map_err(rc));
    }
    let (ca, cb, cc) = (to_csr(&m.a), to_csr(&m.b), to_csr(&m.c));
    let abc = [ca.view(), cb.view(), cc.view()];
    let mut ctx: *mut sys::cg_qap_ctx = std::ptr::null_mut();
    let rc = unsafe {
        // the handle takes `&[Fr]` and returns `Vec<Fr>` as they lie in memory (witness_map_from_matrices below)
        sys::cg_qap_load_form(&mut ctx, abc.as_ptr(), m.num_instance_variables as u64, m.num_constraints as u64,
                              (m.num_instance_variables + m.num_witness_variables) as u64, -1, sys::CG_FORM_MONTGOMERY)
    };
    if rc != 0 {
        return Err(map_err(rc));
    }
    let h = Arc::new(QapHandle(ctx));
    cache.entries.insert(key, (now, h.clone()));
    while cache.entries.len() > QAP_CACHE_MAX {
        let oldest = *cache.entries.iter().min_by_key(|(_, v)| v.0).map(|(k, _)| k).unwrap();
        cache.entries.remove(&oldest); // the Arc drops here, or with the last call still using it
    }
    Ok(h)
}

/// `impl R1CSToQAP` (forks/groth16/src/r1cs_to_qap.rs:49-98).  Usage: `Groth16::<Bn254, GpuReduction>::prove(&pk, circuit, &mut rng)`.
pub struct GpuReduction;

impl R1CSToQAP for GpuReduction {
    // the generator's half is untouched: it runs once per circuit at zksetup time
    fn instance_map_with_evaluation<F: PrimeField, D: EvaluationDomain<F>>(
        cs: ConstraintSystemRef<F>,
        t: &F,
    ) -> Result<(Vec<F>, Vec<F>, Vec<F>, F, usize, usize), SynthesisError> {
        LibsnarkReduction::instance_map_with_evaluation::<F, D>(cs, t)
    }

    fn witness_map_from_matrices<F: PrimeField, D: EvaluationDomain<F>>(
        matrices: &ConstraintMatrices<F>,
        num_inputs: usize,
        num_constraints: usize,
        full_assignment: &[F],
    ) -> Result<Vec<F>, SynthesisError> {
        // The library computes over BN254's scalar field only; any other field keeps the CPU path.  The limbs cross the
        // boundary as they lie in memory, so F must BE ark_bn254::Fr (same type, hence same backend and layout), not only
        // share its modulus.
        if std::any::TypeId::of::<F>() != std::any::TypeId::of::<Fr>() {
            return LibsnarkReduction::witness_map_from_matrices::<F, D>(matrices, num_inputs, num_constraints, full_assignment);
        }
        let m = matrices;
        if num_inputs != m.num_instance_variables || num_constraints != m.num_constraints
            || full_assignment.len() != m.num_instance_variables + m.num_witness_variables
        {
            return Err(SynthesisError::AssignmentMissing);
        }
        let h = qap_for(m)?;
        // SAFETY: F is Fr (TypeId above), so this is the same slice under its own name
        let assignment: &[Fr] = unsafe { std::slice::from_raw_parts(full_assignment.as_ptr() as *const Fr, full_assignment.len()) };
        let w = montgomery_bytes(assignment);
        let d = unsafe { sys::cg_qap_domain_size(h.0) } as usize;
        let mut out = vec![0u8; d * 32];
        let rc = unsafe { sys::cg_qap_witness_map(h.0, w.as_ptr() as *const _, 0, out.as_mut_ptr() as *mut _, 0) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        // domain_size coefficients (r1cs_to_qap.rs:212), already x·2^256 mod r and < r (the library's own results): the limbs
        // ARE the field element, no `from_bigint` (a Montgomery product each) on the way back
        let coeffs: Vec<Fr> = out
            .chunks_exact(32)
            .map(|c| {
                let mut limbs = [0u64; 4];
                for (k, l) in limbs.iter_mut().enumerate() {
                    *l = u64::from_le_bytes(c[k * 8..k * 8 + 8].try_into().unwrap());
                }
                Fr::new_unchecked(BigInt(limbs))
            })
            .collect();
        // SAFETY: F is Fr; the Vec is rebuilt from its own parts under the caller's name for the type
        let mut coeffs = std::mem::ManuallyDrop::new(coeffs);
        Ok(unsafe { Vec::from_raw_parts(coeffs.as_mut_ptr() as *mut F, coeffs.len(), coeffs.capacity()) })
    }

    fn h_query_scalars<F: PrimeField, D: EvaluationDomain<F>>(
        max_power: usize,
        t: F,
        zt: F,
        delta_inverse: F,
    ) -> Result<Vec<F>, SynthesisError> {
        LibsnarkReduction::h_query_scalars::<F, D>(max_power, t, zt, delta_inverse)
    }
}

/// `ConstraintMatrices` of a circom R1CS with column = wire id: the matrices `cs.to_matrices()` yields for
/// `CircomCircuit::generate_constraints` (forks/circom-compat/src/circom/circuit.rs:61-86) when the wire mapping
/// is disabled (builder.rs:63-64).  `constraints` is `circom.r1cs.constraints`.
pub fn matrices_of(num_inputs: usize, num_variables: usize,
                   constraints: &[(Vec<(usize, Fr)>, Vec<(usize, Fr)>, Vec<(usize, Fr)>)]) -> ConstraintMatrices<Fr> {
    let conv = |lc: &Vec<(usize, Fr)>| lc.iter().map(|(j, c)| (*c, *j)).collect::<Vec<_>>();
    let a: Vec<_> = constraints.iter().map(|c| conv(&c.0)).collect();
    let b: Vec<_> = constraints.iter().map(|c| conv(&c.1)).collect();
    let c: Vec<_> = constraints.iter().map(|c| conv(&c.2)).collect();
    ConstraintMatrices {
        num_instance_variables: num_inputs,
        num_witness_variables: num_variables - num_inputs,
        num_constraints: constraints.len(),
        a_num_non_zero: a.iter().map(|r| r.len()).sum(),
        b_num_non_zero: b.iter().map(|r| r.len()).sum(),
        c_num_non_zero: c.iter().map(|r| r.len()).sum(),
        a,
        b,
        c,
    }
}

/// `<G1 as VariableBaseMSM>::msm_bigint` for the show-step sized sums (creds/src/utils.rs:124-138): one-shot.
pub fn msm_g1(bases: &[G1Affine], scalars: &[Fr]) -> Result<G1Affine, SynthesisError> {
    let b = pack_g1(bases);
    let mut sc = Vec::with_capacity(scalars.len() * 32);
    for x in scalars {
        sc.extend_from_slice(&x.into_bigint().to_bytes_le());
    }
    let mut out = [0u8; 64];
    let rc = unsafe {
        sys::cg_msm_g1(b.as_ptr(), sys::CG_FORM_MONTGOMERY, bases.len() as u64, sc.as_ptr(), scalars.len() as u64, 0, out.as_mut_ptr())
    };
    if rc != 0 {
        return Err(map_err(rc));
    }
    if out.iter().all(|v| *v == 0) {
        return Ok(G1Affine::identity());
    }
    let x = Fq::from_le_bytes_mod_order(&out[..32]);
    let y = Fq::from_le_bytes_mod_order(&out[32..]);
    Ok(G1Affine::new_unchecked(x, y))
}

/// `<G2 as VariableBaseMSM>::msm_bigint` for the show-step sized sums over G2 (forks/ark-poly-commit/src/kzg10/mod.rs:196-290
/// commits in G1; the verifier-side G2 sums of creds/src/utils.rs:124-138 callers are this shape): one-shot.
pub fn msm_g2(bases: &[G2Affine], scalars: &[Fr]) -> Result<G2Affine, SynthesisError> {
    let b = pack_g2(bases);
    let mut sc = Vec::with_capacity(scalars.len() * 32);
    for x in scalars {
        sc.extend_from_slice(&x.into_bigint().to_bytes_le());
    }
    let mut out = [0u8; 128];
    let rc = unsafe {
        sys::cg_msm_g2(b.as_ptr(), sys::CG_FORM_MONTGOMERY, bases.len() as u64, sc.as_ptr(), scalars.len() as u64, 0, out.as_mut_ptr())
    };
    if rc != 0 {
        return Err(map_err(rc));
    }
    if out.iter().all(|v| *v == 0) {
        return Ok(G2Affine::identity());
    }
    let x = Fq2::new(Fq::from_le_bytes_mod_order(&out[..32]), Fq::from_le_bytes_mod_order(&out[32..64]));
    let y = Fq2::new(Fq::from_le_bytes_mod_order(&out[64..96]), Fq::from_le_bytes_mod_order(&out[96..]));
    Ok(G2Affine::new_unchecked(x, y))
}

/// A `PreparedVerifyingKey` resident on one GPU (`cg_pvk_load`): what a verifier endpoint keeps per proof spec.
pub struct GpuVerifyingKey {
    h: *mut sys::cg_pvk,
}
unsafe impl Send for GpuVerifyingKey {}
unsafe impl Sync for GpuVerifyingKey {} // calls on one handle serialise inside the library

/// One showing as `ShowGroth16::verify` reads it (creds/src/groth16rand.rs:38-45), borrowed from the caller's struct.
pub struct ShowRef<'a> {
    pub rand_proof: &'a Proof<Bn254>,
    pub com_hidden_inputs: &'a G1Affine,
    pub commited_inputs: &'a [G1Affine],
    pub pok_c: &'a Fr,
    pub pok_s: &'a [Vec<Fr>],
    /// the revealed public inputs, in input order (groth16rand.rs:260-264)
    pub revealed: &'a [Fr],
}

/// What `GpuVerifyingKey::verify_show_batch` returns for one showing.
pub struct ShowOutcome {
    /// `verify_proof_with_prepared_inputs` said true; false covers a rejected and a malformed showing alike
    pub groth16_valid: bool,
    /// the recomputed k_i of `DLogPoK::verify` (creds/src/dlog.rs:137-145), each as the 32 bytes
    /// `add_to_transcript(&mut ts, b"k", &k_i)` appends; all zero when the showing is malformed
    pub k: Vec<[u8; 32]>,
}

impl GpuVerifyingKey {
    /// `pvk_bytes`: the PreparedVerifyingKey as `serialize_uncompressed` writes it (creds/src/utils.rs:186 reads it back).
    pub fn load(pvk_bytes: &[u8], device: i32) -> Result<Self, SynthesisError> {
        let mut h = std::ptr::null_mut();
        let rc = unsafe { sys::cg_pvk_load(&mut h, pvk_bytes.as_ptr(), pvk_bytes.len() as u64, device) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(Self { h })
    }

    /// `true`: one workgroup per proof, for an endpoint that answers one request at a time; `false` (the default): one
    /// lane per proof, for batches (`cg_pvk_set_latency_mode`).  The verdicts are the same.
    pub fn set_latency_mode(&self, on: bool) -> Result<(), SynthesisError> {
        let rc = unsafe { sys::cg_pvk_set_latency_mode(self.h, on as i32) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(())
    }

    /// (group stage, pairing) HIP-event milliseconds of the last verifying call
    pub fn last_kernel_ms(&self) -> Result<(f32, f32), SynthesisError> {
        let (mut a, mut b) = (0f32, 0f32);
        let rc = unsafe { sys::cg_pvk_last_kernel_ms(self.h, &mut a, &mut b) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((a, b))
    }

    /// The GPU share of `ShowGroth16::verify` (groth16rand.rs:232-306) for showings of one proof spec: the Groth16 half
    /// whole, and the recomputed Schnorr commitments of the DLogPoK.  The Merlin transcript stays here on the host:
    /// absorb the bases, `k` and y exactly as dlog.rs:130-152 does, derive the challenge (:166-169) and compare it with
    /// `pok_inputs.c`; a showing is valid when that holds and `groth16_valid` is true ("Verifying showings").
    pub fn verify_show_batch(&self, io_types: &[u8], shows: &[ShowRef]) -> Result<Vec<ShowOutcome>, SynthesisError> {
        let n = shows.len();
        let ShowArrays { n_com, rev, proofs, comh, comm, c, s } = pack_shows(io_types, shows)?;
        let mut verdicts = vec![0u8; n];
        let mut k = vec![0u8; n * (n_com + 1) * 32];
        let rc = unsafe {
            sys::cg_verify_show_batch(self.h, io_types.as_ptr(), io_types.len() as u64, rev.as_ptr(), proofs.as_ptr(), comh.as_ptr(),
                                      comm.as_ptr(), c.as_ptr(), s.as_ptr(), n as u64, verdicts.as_mut_ptr(), k.as_mut_ptr())
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((0..n)
            .map(|i| ShowOutcome {
                groth16_valid: verdicts[i] == sys::CG_VERIFY_ACCEPT,
                k: k[i * (n_com + 1) * 32..(i + 1) * (n_com + 1) * 32].chunks(32).map(|b| b.try_into().unwrap()).collect(),
            })
            .collect())
    }
}

/// The flat arrays of the showing-verifying calls, one row per showing, in the layouts include/crescent_gpu.h states
struct ShowArrays {
    n_com: usize,
    rev: Vec<u8>,
    proofs: Vec<u8>,
    comh: Vec<u8>,
    comm: Vec<u8>,
    c: Vec<u8>,
    s: Vec<u8>,
}

fn pack_shows(io_types: &[u8], shows: &[ShowRef]) -> Result<ShowArrays, SynthesisError> {
    let n_com = io_types.iter().filter(|t| **t == sys::CG_IO_COMMITTED).count();
    let n_hid = io_types.iter().filter(|t| **t == sys::CG_IO_HIDDEN).count();
    let n_rev = io_types.iter().filter(|t| **t == sys::CG_IO_REVEALED).count();
    let (mut rev, mut proofs, mut comh, mut comm, mut c, mut s) = (Vec::new(), Vec::new(), Vec::new(), Vec::new(), Vec::new(), Vec::new());
    for sh in shows {
        let shape_ok = sh.revealed.len() == n_rev
            && sh.commited_inputs.len() == n_com
            && sh.pok_s.len() == n_com + 1
            && sh.pok_s.iter().take(n_com).all(|v| v.len() == 2)
            && sh.pok_s[n_com].len() == n_hid + 1;
        if !shape_ok {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        rev.extend(canonical_bytes(sh.revealed));
        // ark-serialize uncompressed, the layout cg_prove writes and cg_verify_show_batch reads
        sh.rand_proof.serialize_uncompressed(&mut proofs).map_err(|_| SynthesisError::AssignmentMissing)?;
        sh.com_hidden_inputs.serialize_uncompressed(&mut comh).map_err(|_| SynthesisError::AssignmentMissing)?;
        for p in sh.commited_inputs {
            p.serialize_uncompressed(&mut comm).map_err(|_| SynthesisError::AssignmentMissing)?;
        }
        c.extend(canonical_bytes(std::slice::from_ref(sh.pok_c)));
        for si in sh.pok_s {
            s.extend(canonical_bytes(si));
        }
    }
    Ok(ShowArrays { n_com, rev, proofs, comh, comm, c, s })
}

/// One range proof of every showing for `GpuVerifyingKey::verify_showings_batch`: the committed input it is about (counted
/// in committed order), the range key's slot registered for (gamma_abc_g1[pos], delta_g1) of that input, the public value
/// t of each showing (cur_time, or days_to_be_age(age)) and the proofs' rows; `rows.ped_com`, `rows.c` and `rows.rho` are
/// not read: ped_com = commited_inputs[committed_index] - gamma_abc_g1[pos] * t is formed on the GPU.
pub struct ShowRangeLink<'a> {
    pub committed_index: u32,
    pub slot: u32,
    pub shifts: &'a [Fr],
    pub rows: &'a RangeProofRows<'a>,
}

impl GpuVerifyingKey {
    /// The cryptographic checks of `verify_show` / `verify_show_mdl` (creds/src/lib.rs:630-658, :832-890) in one call
    /// (`cg_verify_showings_batch`): `ShowGroth16::verify` whole, its Merlin transcript over `context` included, the link
    /// and `ShowRange::verify` per range proof.  Returns per showing its 1 + links.len() part verdicts (CG_VERIFY_*), the
    /// Groth16 part first; a showing is valid when all of them are CG_VERIFY_ACCEPT.  Not covered: the SHA-256 of revealed
    /// preimages, the freshness test on cur_time and the device proof ("Verifying whole showings").
    pub fn verify_showings_batch(&self, range_key: Option<&GpuRangeVerifyingKey>, io_types: &[u8], context: Option<&[u8]>, shows: &[ShowRef],
                                 links: &[ShowRangeLink]) -> Result<Vec<Vec<u8>>, SynthesisError> {
        let n = shows.len();
        let a = pack_shows(io_types, shows)?;
        if !links.is_empty() && range_key.is_none() {
            return Err(SynthesisError::AssignmentMissing);
        }
        let mut shifts = vec![0u8; n * links.len() * 32];
        let (mut c_links, mut c_rows, mut keep) = (Vec::new(), Vec::new(), Vec::new());
        for (j, l) in links.iter().enumerate() {
            let r = l.rows;
            if l.shifts.len() != n || r.com_f.len() != n * 64 || r.com_g.len() != n * 64 || r.com_q.len() != n * 64 || r.evals.len() != n * 96
                || r.proofs.len() != n * 288 || r.randomizers.len() != 2 * n || r.pok_c.len() != n || r.pok_s.len() != n * sys::CG_RANGE_N_RESP
            {
                return Err(SynthesisError::MalformedVerifyingKey);
            }
            for (i, t) in canonical_bytes(l.shifts).chunks(32).enumerate() {
                shifts[(i * links.len() + j) * 32..(i * links.len() + j + 1) * 32].copy_from_slice(t);
            }
            let zb: Vec<u8> = r.randomizers.iter().flat_map(|z| z.to_le_bytes()).collect();
            keep.push((zb, canonical_bytes(r.pok_c), canonical_bytes(r.pok_s)));
            c_links.push(sys::cg_show_range_link { committed_index: l.committed_index, slot: l.slot });
        }
        for (l, (zb, pc, ps)) in links.iter().zip(keep.iter()) {
            let r = l.rows;
            c_rows.push(sys::cg_range_rows { com_f: r.com_f.as_ptr(), com_g: r.com_g.as_ptr(), com_q: r.com_q.as_ptr(), evals: r.evals.as_ptr(),
                                             proofs: r.proofs.as_ptr(), randomizers: zb.as_ptr(), pok_c: pc.as_ptr(), pok_s: ps.as_ptr() });
        }
        let ctx = context.unwrap_or(&[]);
        let width = 1 + links.len();
        let (mut verdicts, mut parts) = (vec![0u8; n], vec![0u8; n * width]);
        let rc = unsafe {
            sys::cg_verify_showings_batch(self.h, range_key.map_or(std::ptr::null_mut(), |k| k.h), io_types.as_ptr(), io_types.len() as u64,
                                          if ctx.is_empty() { std::ptr::null() } else { ctx.as_ptr() }, ctx.len() as u64, 0, a.rev.as_ptr(),
                                          a.proofs.as_ptr(), a.comh.as_ptr(), a.comm.as_ptr(), a.c.as_ptr(), a.s.as_ptr(), links.len() as u32,
                                          c_links.as_ptr(), shifts.as_ptr(), c_rows.as_ptr(), n as u64, verdicts.as_mut_ptr(), parts.as_mut_ptr())
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(parts.chunks(width).map(|p| p.to_vec()).collect())
    }

    /// The creating side's link, `com.m -= t; com.c -= bases[0] * t` before `show_range` (creds/src/lib.rs:370-372, :468-470,
    /// :505-507), for n openings (m, r) of the committed input `input_index` (`cg_show_shift_batch`).  Returns (openings n x
    /// 2 x 32 B, ped_com n x 64 B, status n x CG_SHOW_*) in the layouts `GpuRangeKey::prove_batch` takes.
    pub fn show_shift_batch(&self, input_index: u32, openings: &[(Fr, Fr)], commitments: &[G1Affine], shifts: &[Fr]) -> Result<(Vec<u8>, Vec<u8>, Vec<u8>), SynthesisError> {
        let n = openings.len();
        if commitments.len() != n || shifts.len() != n {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let flat: Vec<Fr> = openings.iter().flat_map(|(m, r)| [*m, *r]).collect();
        let (ob, sb) = (canonical_bytes(&flat), canonical_bytes(shifts));
        let mut cb = Vec::with_capacity(n * 64);
        for p in commitments {
            p.serialize_uncompressed(&mut cb).map_err(|_| SynthesisError::AssignmentMissing)?;
        }
        let (mut out, mut ped, mut status) = (vec![0u8; n * 64], vec![0u8; n * 64], vec![0u8; n]);
        let rc = unsafe {
            sys::cg_show_shift_batch(self.h, input_index, ob.as_ptr(), cb.as_ptr(), sb.as_ptr(), n as u64, out.as_mut_ptr(), ped.as_mut_ptr(),
                                     status.as_mut_ptr())
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((out, ped, status))
    }

    /// The BN254 half of `DeviceProof::verify` (creds/src/device.rs:168-213; called from creds/src/lib.rs:660-680, :893-913) for
    /// n device-bound showings of one layout in one call (`cg_device_link_verify_batch`): pi0 with its equal-scalar pair, the
    /// SHA-256 challenge over the commitments' text forms, the recombination and pi1.  `committed` is the showing's own
    /// n x n_committed x 64 B array, as `verify_showings_batch` takes it; `pos0` and `pos1` are the input indices of
    /// `device_key_0_value` and `device_key_1_value`; every array of `rows` holds n rows in the header's layout and every h_Q
    /// has `h_len` bytes.  Returns (verdicts n x CG_VERIFY_*, part verdicts n x 2, e n x 32 B: e1_bytes ‖ e2_bytes, which the
    /// host passes on to `ECDSAProof::verify` with m).  pi2 stays with the host.
    pub fn device_link_verify_batch(&self, io_types: &[u8], pos0: u32, pos1: u32, committed: &[u8], rows: &DeviceLinkRows, h_len: u32) -> Result<(Vec<u8>, Vec<u8>, Vec<u8>), SynthesisError> {
        let n = rows.com1.len() / 64;
        let n_com = io_types.iter().filter(|&&t| t == 2).count();
        if rows.com1.len() != n * 64 || rows.comz.len() != n * 64 || rows.h_q.len() != n * h_len as usize || rows.m.len() != n * 32 || rows.pi0_c.len() != n * 32
            || rows.pi0_s.len() != n * 128 || rows.pi1_c.len() != n * 32 || rows.pi1_s.len() != n * 96 || committed.len() != n * n_com * 64
        {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let c_rows = sys::cg_device_link_rows { com1: rows.com1.as_ptr(), comz: rows.comz.as_ptr(), h_q: rows.h_q.as_ptr(), m: rows.m.as_ptr(),
                                                pi0_c: rows.pi0_c.as_ptr(), pi0_s: rows.pi0_s.as_ptr(), pi1_c: rows.pi1_c.as_ptr(), pi1_s: rows.pi1_s.as_ptr() };
        let (mut verdicts, mut parts, mut e) = (vec![0u8; n], vec![0u8; n * 2], vec![0u8; n * 32]);
        let rc = unsafe {
            sys::cg_device_link_verify_batch(self.h, io_types.as_ptr(), io_types.len() as u64, pos0, pos1, committed.as_ptr(), &c_rows, h_len, n as u64,
                                             verdicts.as_mut_ptr(), parts.as_mut_ptr(), e.as_mut_ptr())
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((verdicts, parts, e))
    }

    /// HIP-event milliseconds of the four kernels of the last `device_link_verify_batch` on this key
    /// (`cg_device_link_last_kernel_ms`): the digest and scalar stage, the terms, the sums, the two transcripts.
    pub fn device_link_last_kernel_ms(&self) -> Result<[f32; 4], SynthesisError> {
        let mut ms = [0f32; 4];
        let rc = unsafe { sys::cg_device_link_last_kernel_ms(self.h, ms.as_mut_ptr()) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(ms)
    }

    /// The BN254 half of `DeviceProof::prove` (creds/src/device.rs:104-160) for n device-bound showings of one layout in one
    /// call (`cg_device_link_prove_batch`), short of `compute_hQ` (see `device_link_prove_hq_batch`) and of pi2: comz, the re-committed com1, pi0, the SHA-256
    /// challenge, m, lhs1 and pi1.  `committed` is the showing's own n x n_committed x 64 B array, as `create_showings_batch`
    /// returned it; `openings` holds n x (q0, r0, q1, r1_orig) and `rand` n x `CG_DEVICE_LINK_N_RAND` canonical scalars in the
    /// header's order; `h_q` n x `h_len` bytes.  Returns (the rows, with the caller's h_q, as `device_link_verify_batch` takes
    /// them; e n x 32 B: e1_bytes ‖ e2_bytes, which the host hands to `ECDSAProof::prove` with m and its own z; status n x
    /// CG_SHOW_MADE / CG_SHOW_MALFORMED, a malformed row being zero bytes throughout).
    pub fn device_link_prove_batch(&self, io_types: &[u8], pos0: u32, pos1: u32, committed: &[u8], openings: &[u8], rand: &[u8], h_q: &[u8], h_len: u32) -> Result<(DeviceLinkRows, Vec<u8>, Vec<u8>), SynthesisError> {
        let n = openings.len() / 128;
        let n_com = io_types.iter().filter(|&&t| t == 2).count();
        if openings.len() != n * 128 || rand.len() != n * 32 * sys::CG_DEVICE_LINK_N_RAND || h_q.len() != n * h_len as usize || committed.len() != n * n_com * 64 {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let mut rows = DeviceLinkRows { com1: vec![0u8; n * 64], comz: vec![0u8; n * 64], h_q: h_q.to_vec(), m: vec![0u8; n * 32], pi0_c: vec![0u8; n * 32],
                                        pi0_s: vec![0u8; n * 128], pi1_c: vec![0u8; n * 32], pi1_s: vec![0u8; n * 96] };
        let made = sys::cg_device_link_made { com1: rows.com1.as_mut_ptr(), comz: rows.comz.as_mut_ptr(), m: rows.m.as_mut_ptr(), pi0_c: rows.pi0_c.as_mut_ptr(),
                                              pi0_s: rows.pi0_s.as_mut_ptr(), pi1_c: rows.pi1_c.as_mut_ptr(), pi1_s: rows.pi1_s.as_mut_ptr() };
        let (mut e, mut status) = (vec![0u8; n * 32], vec![0u8; n]);
        let rc = unsafe {
            sys::cg_device_link_prove_batch(self.h, io_types.as_ptr(), io_types.len() as u64, pos0, pos1, committed.as_ptr(), openings.as_ptr(), rand.as_ptr(),
                                            h_q.as_ptr(), h_len, n as u64, &made, e.as_mut_ptr(), status.as_mut_ptr())
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((rows, e, status))
    }

    /// `device_link_prove_batch` with `compute_hQ` in the same call (`cg_device_link_prove_hq_batch`): h_Q is computed on the
    /// GPU from q0 and q1 (`openings`) and z (`rand[0]`) and comes back in the rows' `h_q`, 32 bytes per row.  The host computes
    /// nothing before the call and hands m, e and z to `ECDSAProof::prove` after it.
    pub fn device_link_prove_hq_batch(&self, io_types: &[u8], pos0: u32, pos1: u32, committed: &[u8], openings: &[u8], rand: &[u8]) -> Result<(DeviceLinkRows, Vec<u8>, Vec<u8>), SynthesisError> {
        let n = openings.len() / 128;
        let n_com = io_types.iter().filter(|&&t| t == 2).count();
        if openings.len() != n * 128 || rand.len() != n * 32 * sys::CG_DEVICE_LINK_N_RAND || committed.len() != n * n_com * 64 {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let mut rows = DeviceLinkRows { com1: vec![0u8; n * 64], comz: vec![0u8; n * 64], h_q: vec![0u8; n * 32], m: vec![0u8; n * 32], pi0_c: vec![0u8; n * 32],
                                        pi0_s: vec![0u8; n * 128], pi1_c: vec![0u8; n * 32], pi1_s: vec![0u8; n * 96] };
        let made = sys::cg_device_link_made { com1: rows.com1.as_mut_ptr(), comz: rows.comz.as_mut_ptr(), m: rows.m.as_mut_ptr(), pi0_c: rows.pi0_c.as_mut_ptr(),
                                              pi0_s: rows.pi0_s.as_mut_ptr(), pi1_c: rows.pi1_c.as_mut_ptr(), pi1_s: rows.pi1_s.as_mut_ptr() };
        let (mut e, mut status) = (vec![0u8; n * 32], vec![0u8; n]);
        let rc = unsafe {
            sys::cg_device_link_prove_hq_batch(self.h, io_types.as_ptr(), io_types.len() as u64, pos0, pos1, committed.as_ptr(), openings.as_ptr(), rand.as_ptr(),
                                               n as u64, &made, e.as_mut_ptr(), status.as_mut_ptr(), rows.h_q.as_mut_ptr())
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((rows, e, status))
    }

    /// `compute_hQ` (ecdsa-pop/src/lib.rs:308-320) for n rows of (q0, q1, z), 3 x 32 B canonical Fr (`cg_hq_batch`).  Returns
    /// (h_Q n x 32 B big-endian, as `device_link_prove_batch` takes them with h_len = 32; status n x CG_SHOW_MADE /
    /// CG_SHOW_MALFORMED, a row with a scalar >= r being zero bytes).
    pub fn hq_batch(&self, q: &[u8]) -> Result<(Vec<u8>, Vec<u8>), SynthesisError> {
        let n = q.len() / 96;
        if q.len() != n * 96 {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let (mut h_q, mut status) = (vec![0u8; n * 32], vec![0u8; n]);
        let rc = unsafe { sys::cg_hq_batch(self.h, q.as_ptr(), n as u64, h_q.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((h_q, status))
    }

    /// Poseidon of width 3 over P-256's base field on n states of 3 x 32 B canonical little-endian elements
    /// (`cg_poseidon_p256_permute_batch`): (the permuted states, status; a row with an element >= p is malformed and zero).
    pub fn poseidon_p256_permute_batch(&self, states: &[u8]) -> Result<(Vec<u8>, Vec<u8>), SynthesisError> {
        let n = states.len() / 96;
        if states.len() != n * 96 {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let (mut out, mut status) = (vec![0u8; n * 96], vec![0u8; n]);
        let rc = unsafe { sys::cg_poseidon_p256_permute_batch(self.h, states.as_ptr(), n as u64, out.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((out, status))
    }

    /// `ECDSACircuitPublicInputs::compute_TU` (ecdsa-pop/src/lib.rs:217-240) for n rows (`cg_p256_tu_batch`): `r_xy` n x 64 B
    /// (R as x ‖ y) and `digest` n x 32 B, every P-256 quantity 32 bytes big-endian.  Returns (T n x 64 B, U n x 64 B, status
    /// n x CG_SHOW_MADE / CG_SHOW_MALFORMED): the public inputs `ECDSAProof::verify` hands its circuit.  A malformed row - a
    /// coordinate >= p, R off the curve, R.x = 0 mod n, where the reference panics - is zero bytes; so is the identity.
    pub fn p256_tu_batch(&self, r_xy: &[u8], digest: &[u8]) -> Result<(Vec<u8>, Vec<u8>, Vec<u8>), SynthesisError> {
        let n = r_xy.len() / 64;
        if r_xy.len() != n * 64 || digest.len() != n * 32 {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let (mut t, mut u, mut status) = (vec![0u8; n * 64], vec![0u8; n * 64], vec![0u8; n]);
        let rc = unsafe { sys::cg_p256_tu_batch(self.h, r_xy.as_ptr(), digest.as_ptr(), n as u64, t.as_mut_ptr(), u.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((t, u, status))
    }

    /// `compute_RTU` (ecdsa-pop/src/lib.rs:180-215) for n rows (`cg_p256_rtu_batch`): `q_xy` n x 64 B (the device's public
    /// key), `sig` n x 64 B (r ‖ s), `digest` n x 32 B.  Returns (R, T, U, each n x 64 B, status n): CG_SHOW_MADE,
    /// CG_SHOW_MALFORMED or `sys::CG_P256_BAD_SIGNATURE`, where the reference panics on its assertion; every output of a row
    /// that is not made is zero bytes.  This is the only place where the device's signature is checked.
    pub fn p256_rtu_batch(&self, q_xy: &[u8], sig: &[u8], digest: &[u8]) -> Result<(Vec<u8>, Vec<u8>, Vec<u8>, Vec<u8>), SynthesisError> {
        let n = q_xy.len() / 64;
        if q_xy.len() != n * 64 || sig.len() != n * 64 || digest.len() != n * 32 {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let (mut r, mut t, mut u, mut status) = (vec![0u8; n * 64], vec![0u8; n * 64], vec![0u8; n * 64], vec![0u8; n]);
        let rc = unsafe {
            sys::cg_p256_rtu_batch(self.h, q_xy.as_ptr(), sig.as_ptr(), digest.as_ptr(), n as u64, r.as_mut_ptr(), t.as_mut_ptr(), u.as_mut_ptr(),
                                   status.as_mut_ptr())
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((r, t, u, status))
    }

    /// (`cg_p256_last_kernel_ms`) HIP-event milliseconds of the three kernels of the last `p256_tu_batch` or `p256_rtu_batch`
    /// on this key - the scalar stage, the terms, the finishing stage - and how often the table of P-256's generator was
    /// uploaded to it (0 or 1).
    pub fn p256_last_kernel_ms(&self) -> Result<([f32; 3], u32), SynthesisError> {
        let (mut ms, mut uploads) = ([0f32; 3], 0u32);
        let rc = unsafe { sys::cg_p256_last_kernel_ms(self.h, ms.as_mut_ptr(), &mut uploads) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((ms, uploads))
    }

    /// (`cg_hq_last_kernel_ms`) HIP-event milliseconds of the kernel of the last `hq_batch` or `poseidon_p256_permute_batch`
    /// on this key and of the h_Q kernel of its last `device_link_prove_hq_batch`; and how often the Poseidon constants were
    /// uploaded to it (0 or 1).
    pub fn hq_last_kernel_ms(&self) -> Result<([f32; 2], u32), SynthesisError> {
        let (mut ms, mut uploads) = ([0f32; 2], 0u32);
        let rc = unsafe { sys::cg_hq_last_kernel_ms(self.h, ms.as_mut_ptr(), &mut uploads) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((ms, uploads))
    }

    /// HIP-event milliseconds of the six kernels of the last `device_link_prove_batch` on this key
    /// (`cg_device_link_prove_last_kernel_ms`): the checks, the walks, the sums, pi0 with the digest, lhs1, pi1.
    pub fn device_link_prove_last_kernel_ms(&self) -> Result<[f32; 6], SynthesisError> {
        let mut ms = [0f32; 6];
        let rc = unsafe { sys::cg_device_link_prove_last_kernel_ms(self.h, ms.as_mut_ptr()) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(ms)
    }

    /// `create_show_proof`'s `show_groth16` and `show_range` steps (creds/src/lib.rs:364-373, :468-471, :505-509) for `n`
    /// client states of one proof spec in one call (`cg_create_showings_batch`): the re-randomised proof, the commitments,
    /// `DLogPoK::prove` whole with its Merlin transcript over `context`, and per link the shift by `shifts` and
    /// `prove_n_bits` whole.  `inputs`: n x io_types.len(); `rand`: n x `cg_show_rand_count` scalars drawn by the caller in
    /// the header's order (r1, r2, the r_i, z, the nonces) - keep the r_i and z as `committed_input_openings` /
    /// `input_com_randomness`; `links[j]`: the committed input and the slot of `range_key` (`GpuRangeKey::add_bases`);
    /// `shifts`: n x links.len(); `range_rand`: n x links.len() x CG_RANGE_N_RAND.  The opening of a link is the showing's
    /// own: (inputs[pos], r_ci).  INTEGRATION.md, "Creating whole showings".
    #[allow(clippy::too_many_arguments)]
    pub fn create_showings_batch(&self, range_key: Option<&GpuRangeKey>, io_types: &[u8], context: Option<&[u8]>, proofs: &[Proof<Bn254>],
                                 inputs: &[Fr], rand: &[Fr], links: &[(u32, u32)], shifts: &[Fr], range_rand: &[Fr])
                                 -> Result<ShowingsMade, SynthesisError> {
        let n = proofs.len();
        let n_com = io_types.iter().filter(|t| **t == sys::CG_IO_COMMITTED).count();
        let mut n_rand = 0u64;
        let rc = unsafe { sys::cg_show_rand_count(io_types.as_ptr(), io_types.len() as u64, &mut n_rand) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        if !links.is_empty() && range_key.is_none() {
            return Err(SynthesisError::AssignmentMissing);
        }
        if inputs.len() != n * io_types.len() || rand.len() != n * n_rand as usize || shifts.len() != n * links.len()
            || range_rand.len() != n * links.len() * sys::CG_RANGE_N_RAND
        {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let n_resp = n_rand as usize - 3 - n_com;
        let mut pb = Vec::with_capacity(n * 256);
        for p in proofs {
            p.serialize_uncompressed(&mut pb).map_err(|_| SynthesisError::AssignmentMissing)?;
        }
        let (ib, rb, sb, rrb) = (canonical_bytes(inputs), canonical_bytes(rand), canonical_bytes(shifts), canonical_bytes(range_rand));
        let c_links: Vec<sys::cg_show_range_link> = links.iter().map(|&(committed_index, slot)| sys::cg_show_range_link { committed_index, slot }).collect();
        let mut out = ShowingsMade {
            rand_proofs: vec![0u8; n * 256],
            com_hidden: vec![0u8; n * 64],
            committed: vec![0u8; n * n_com * 64 + 64],
            pok_c: vec![0u8; n * 32],
            pok_s: vec![0u8; n * n_resp * 32],
            ranges: links
                .iter()
                .map(|_| RangeProofsMade {
                    com_f: vec![0u8; n * 64],
                    com_g: vec![0u8; n * 64],
                    com_q: vec![0u8; n * 64],
                    evals: vec![0u8; n * 96],
                    proofs: vec![0u8; n * 288],
                    pok_c: vec![0u8; n * 32],
                    pok_s: vec![0u8; n * sys::CG_RANGE_N_RESP * 32],
                    challenges: vec![0u8; n * 96],
                    status: vec![0u8; n],
                })
                .collect(),
            status: vec![0u8; n],
        };
        let c_made: Vec<sys::cg_range_made> = out
            .ranges
            .iter_mut()
            .map(|r| sys::cg_range_made {
                com_f: r.com_f.as_mut_ptr(),
                com_g: r.com_g.as_mut_ptr(),
                com_q: r.com_q.as_mut_ptr(),
                evals: r.evals.as_mut_ptr(),
                proofs: r.proofs.as_mut_ptr(),
                pok_c: r.pok_c.as_mut_ptr(),
                pok_s: r.pok_s.as_mut_ptr(),
                challenges: r.challenges.as_mut_ptr(),
            })
            .collect();
        let ctx = context.unwrap_or(&[]);
        let width = 1 + links.len();
        let mut parts = vec![0u8; n * width];
        let rc = unsafe {
            sys::cg_create_showings_batch(self.h, range_key.map_or(std::ptr::null_mut(), |k| k.h), io_types.as_ptr(), io_types.len() as u64,
                                          if ctx.is_empty() { std::ptr::null() } else { ctx.as_ptr() }, ctx.len() as u64, 0, pb.as_ptr(), ib.as_ptr(),
                                          rb.as_ptr(), links.len() as u32, c_links.as_ptr(), sb.as_ptr(), rrb.as_ptr(), n as u64,
                                          out.rand_proofs.as_mut_ptr(), out.com_hidden.as_mut_ptr(), out.committed.as_mut_ptr(),
                                          out.pok_c.as_mut_ptr(), out.pok_s.as_mut_ptr(), c_made.as_ptr(), out.status.as_mut_ptr(), parts.as_mut_ptr())
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        out.committed.truncate(n * n_com * 64);
        for (j, r) in out.ranges.iter_mut().enumerate() {
            for i in 0..n {
                r.status[i] = parts[i * width + 1 + j];
            }
        }
        Ok(out)
    }

    /// Diagnostic (`cg_pvk_set_showings_overlap`): whether `verify_showings_batch` and `create_showings_batch` start the range
    /// half beside the Groth16 half (the default) or behind it
    pub fn set_showings_overlap(&self, on: bool) -> Result<(), SynthesisError> {
        let rc = unsafe { sys::cg_pvk_set_showings_overlap(self.h, on as i32) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(())
    }
}

/// What `GpuVerifyingKey::create_showings_batch` returns: the Groth16 part in the layouts of `show_commit_batch` and
/// `show_respond_batch`, per link the rows of `GpuRangeKey::prove_batch` (their `status` is the link's part status), and one
/// CG_SHOW_* byte per client state: CG_SHOW_MADE only if every part was made.  A part that was not made has zero bytes.
pub struct ShowingsMade {
    pub rand_proofs: Vec<u8>,
    pub com_hidden: Vec<u8>,
    pub committed: Vec<u8>,
    pub pok_c: Vec<u8>,
    pub pok_s: Vec<u8>,
    pub ranges: Vec<RangeProofsMade>,
    pub status: Vec<u8>,
}

/// What `GpuVerifyingKey::show_commit_batch` returns: the flat arrays of `cg_show_commit_batch`, one row per client state.
pub struct ShowCommitments {
    /// n x 256 B: A' | B' | C'' ark-serialize uncompressed (`Proof::deserialize_uncompressed_unchecked` reads a row back)
    pub rand_proofs: Vec<u8>,
    /// n x 64 B: com_hidden_inputs
    pub com_hidden: Vec<u8>,
    /// n x n_committed x 64 B: commited_inputs
    pub committed: Vec<u8>,
    /// n x (n_committed + 1) x 32 B: the k_i as `add_to_transcript(&mut ts, b"k", &k_i)` appends them
    pub k: Vec<u8>,
    /// n x CG_SHOW_MADE / CG_SHOW_MALFORMED
    pub status: Vec<u8>,
}

impl GpuVerifyingKey {
    /// The GPU share of `ClientState::show_groth16` (groth16rand.rs:100-187) for `n` client states of one proof spec:
    /// `rerandomize_proof`, the Pedersen commitments, com_hidden_inputs, the correction of C and the k_i of
    /// `DLogPoK::prove`.  `inputs`: n x io_types.len() (`ClientState.inputs`); `rand`: n x `cg_show_rand_count` scalars
    /// drawn by the caller in the header's order (r1, r2, the r_i, z, the nonces).  The Merlin transcript stays here on
    /// the host: absorb the bases, `k` and y as dlog.rs:56-99 does, derive c, then call `show_respond_batch`, and keep
    /// the r_i and z as `committed_input_openings` / `input_com_randomness` ("Creating showings").
    pub fn show_commit_batch(&self, io_types: &[u8], proofs: &[Proof<Bn254>], inputs: &[Fr], rand: &[Fr]) -> Result<ShowCommitments, SynthesisError> {
        let n = proofs.len();
        let n_com = io_types.iter().filter(|t| **t == sys::CG_IO_COMMITTED).count();
        let mut n_rand = 0u64;
        let rc = unsafe { sys::cg_show_rand_count(io_types.as_ptr(), io_types.len() as u64, &mut n_rand) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        if inputs.len() != n * io_types.len() || rand.len() != n * n_rand as usize {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let mut pb = Vec::with_capacity(n * 256);
        for p in proofs {
            p.serialize_uncompressed(&mut pb).map_err(|_| SynthesisError::AssignmentMissing)?;
        }
        let (ib, rb) = (canonical_bytes(inputs), canonical_bytes(rand));
        let mut out = ShowCommitments {
            rand_proofs: vec![0u8; n * 256],
            com_hidden: vec![0u8; n * 64],
            committed: vec![0u8; n * n_com * 64 + 64],
            k: vec![0u8; n * (n_com + 1) * 32],
            status: vec![0u8; n],
        };
        let rc = unsafe {
            sys::cg_show_commit_batch(self.h, io_types.as_ptr(), io_types.len() as u64, pb.as_ptr(), ib.as_ptr(), rb.as_ptr(), n as u64,
                                      out.rand_proofs.as_mut_ptr(), out.com_hidden.as_mut_ptr(), out.committed.as_mut_ptr(),
                                      out.k.as_mut_ptr(), out.status.as_mut_ptr())
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        out.committed.truncate(n * n_com * 64);
        Ok(out)
    }

    /// The responses of `DLogPoK::prove` (dlog.rs:101-109) for the challenges the host's transcript produced: n x n_resp
    /// canonical 32-byte scalars in the order `pok_inputs.s` flattens to.  Host arithmetic only; `inputs`, `rand` and
    /// `status` are those of `show_commit_batch` (a state that is not CG_SHOW_MADE gets zeros).
    pub fn show_respond_batch(io_types: &[u8], inputs: &[Fr], rand: &[Fr], pok_c: &[Fr], status: &[u8]) -> Result<Vec<u8>, SynthesisError> {
        let n = pok_c.len();
        let n_com = io_types.iter().filter(|t| **t == sys::CG_IO_COMMITTED).count();
        let mut n_rand = 0u64;
        let rc = unsafe { sys::cg_show_rand_count(io_types.as_ptr(), io_types.len() as u64, &mut n_rand) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        if inputs.len() != n * io_types.len() || rand.len() != n * n_rand as usize || status.len() != n {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let n_resp = n_rand as usize - 3 - n_com;
        let (ib, rb, cb) = (canonical_bytes(inputs), canonical_bytes(rand), canonical_bytes(pok_c));
        let mut s = vec![0u8; n * n_resp * 32];
        let rc = unsafe {
            sys::cg_show_respond_batch(io_types.as_ptr(), io_types.len() as u64, ib.as_ptr(), rb.as_ptr(), cb.as_ptr(), status.as_ptr(),
                                       n as u64, s.as_mut_ptr())
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(s)
    }
}

impl Drop for GpuVerifyingKey {
    fn drop(&mut self) {
        unsafe { sys::cg_pvk_free(self.h) }
    }
}

/// A KZG key resident on the GPU for creating range proofs (`RangeProof::prove_n_bits`, creds/src/rangeproof.rs:114-339)
/// in batches: three GPU calls around the host's transcripts, then the responses ("Creating range proofs").
pub struct GpuRangeKey {
    h: *mut sys::cg_range_pk,
}
unsafe impl Send for GpuRangeKey {}
unsafe impl Sync for GpuRangeKey {} // calls on one handle serialise inside the library

/// What `commit_batch` returns: com_f, com_g n x 64 B uncompressed; ts n x 4 x 32 B compressed (com_f, com_g, k_0, k_1)
pub struct RangeCommitments {
    pub com_f: Vec<u8>,
    pub com_g: Vec<u8>,
    pub ts: Vec<u8>,
    pub status: Vec<u8>,
}
/// com_q n x 64 B uncompressed; ts_q n x 32 B compressed
pub struct RangeQuotients {
    pub com_q: Vec<u8>,
    pub ts_q: Vec<u8>,
    pub status: Vec<u8>,
}
/// evals n x 3 x 32 B (eval_g, eval_gw, eval_w_hat); proofs n x 3 x 96 B (W uncompressed, then random_v)
pub struct RangeOpenings {
    pub evals: Vec<u8>,
    pub proofs: Vec<u8>,
    pub status: Vec<u8>,
}

impl GpuRangeKey {
    /// `range_pk_bytes`: range_pk.bin as `write_to_file` writes it (creds/src/lib.rs:241); `n_bits`: 32 in the product
    pub fn load(range_pk_bytes: &[u8], n_bits: u32) -> Result<Self, SynthesisError> {
        let mut h = std::ptr::null_mut();
        let rc = unsafe { sys::cg_range_pk_load(&mut h, range_pk_bytes.as_ptr(), range_pk_bytes.len() as u64, n_bits, -1) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(GpuRangeKey { h })
    }

    /// Registers the Pedersen bases of one range-checked input (groth16rand.rs:135-139) and returns their slot.
    pub fn add_bases(&self, gamma_abc_point: &G1Affine, delta_g1: &G1Affine) -> Result<u32, SynthesisError> {
        let mut b = Vec::with_capacity(128);
        for p in [gamma_abc_point, delta_g1] {
            p.serialize_uncompressed(&mut b).map_err(|_| SynthesisError::AssignmentMissing)?;
        }
        let mut slot = 0u32;
        let rc = unsafe { sys::cg_range_pk_add_bases(self.h, b.as_ptr(), &mut slot) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(slot)
    }

    /// `openings`: n x (m, r); `rand`: n x 18 scalars in the header's order
    pub fn commit_batch(&self, slot: u32, openings: &[Fr], rand: &[Fr]) -> Result<RangeCommitments, SynthesisError> {
        let n = openings.len() / 2;
        if openings.len() != 2 * n || rand.len() != n * sys::CG_RANGE_N_RAND {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let (ob, rb) = (canonical_bytes(openings), canonical_bytes(rand));
        let mut out = RangeCommitments { com_f: vec![0u8; n * 64], com_g: vec![0u8; n * 64], ts: vec![0u8; n * 128], status: vec![0u8; n] };
        let rc = unsafe {
            sys::cg_range_commit_batch(self.h, slot, ob.as_ptr(), rb.as_ptr(), n as u64, out.com_f.as_mut_ptr(), out.com_g.as_mut_ptr(),
                                       out.ts.as_mut_ptr(), out.status.as_mut_ptr())
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(out)
    }

    pub fn quotient_batch(&self, openings: &[Fr], rand: &[Fr], c: &[Fr]) -> Result<RangeQuotients, SynthesisError> {
        let n = c.len();
        if openings.len() != 2 * n || rand.len() != n * sys::CG_RANGE_N_RAND {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let (ob, rb, cb) = (canonical_bytes(openings), canonical_bytes(rand), canonical_bytes(c));
        let mut out = RangeQuotients { com_q: vec![0u8; n * 64], ts_q: vec![0u8; n * 32], status: vec![0u8; n] };
        let rc = unsafe {
            sys::cg_range_quotient_batch(self.h, ob.as_ptr(), rb.as_ptr(), cb.as_ptr(), n as u64, out.com_q.as_mut_ptr(),
                                         out.ts_q.as_mut_ptr(), out.status.as_mut_ptr())
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(out)
    }

    pub fn open_batch(&self, openings: &[Fr], rand: &[Fr], c: &[Fr], rho: &[Fr]) -> Result<RangeOpenings, SynthesisError> {
        let n = c.len();
        if openings.len() != 2 * n || rand.len() != n * sys::CG_RANGE_N_RAND || rho.len() != n {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let (ob, rb, cb, hb) = (canonical_bytes(openings), canonical_bytes(rand), canonical_bytes(c), canonical_bytes(rho));
        let mut out = RangeOpenings { evals: vec![0u8; n * 96], proofs: vec![0u8; n * 288], status: vec![0u8; n] };
        let rc = unsafe {
            sys::cg_range_open_batch(self.h, ob.as_ptr(), rb.as_ptr(), cb.as_ptr(), hb.as_ptr(), n as u64, out.evals.as_mut_ptr(),
                                     out.proofs.as_mut_ptr(), out.status.as_mut_ptr())
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(out)
    }

    /// The DLEQ's responses (dlog.rs:101-109): n x 6 canonical 32-byte scalars, s_00 s_01 | s_10..s_13.  Host arithmetic only.
    pub fn respond_batch(openings: &[Fr], rand: &[Fr], c_dleq: &[Fr], status: &[u8]) -> Result<Vec<u8>, SynthesisError> {
        let n = c_dleq.len();
        if openings.len() != 2 * n || rand.len() != n * sys::CG_RANGE_N_RAND || status.len() != n {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let (ob, rb, cb) = (canonical_bytes(openings), canonical_bytes(rand), canonical_bytes(c_dleq));
        let mut s = vec![0u8; n * sys::CG_RANGE_N_RESP * 32];
        let rc = unsafe { sys::cg_range_respond_batch(ob.as_ptr(), rb.as_ptr(), cb.as_ptr(), status.as_ptr(), n as u64, s.as_mut_ptr()) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(s)
    }

    /// `RangeProof::prove_n_bits` in one call (`cg_range_prove_batch`): the three phases with the library's Merlin between
    /// them, on the GPU.  `ped_com`: n x 64 B uncompressed, the commitments the openings open.
    pub fn prove_batch(&self, slot: u32, openings: &[Fr], ped_com: &[u8], rand: &[Fr]) -> Result<RangeProofsMade, SynthesisError> {
        let n = openings.len() / 2;
        if openings.len() != 2 * n || ped_com.len() != n * 64 || rand.len() != n * sys::CG_RANGE_N_RAND {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let (ob, rb) = (canonical_bytes(openings), canonical_bytes(rand));
        let mut out = RangeProofsMade {
            com_f: vec![0u8; n * 64],
            com_g: vec![0u8; n * 64],
            com_q: vec![0u8; n * 64],
            evals: vec![0u8; n * 96],
            proofs: vec![0u8; n * 288],
            pok_c: vec![0u8; n * 32],
            pok_s: vec![0u8; n * sys::CG_RANGE_N_RESP * 32],
            challenges: vec![0u8; n * 96],
            status: vec![0u8; n],
        };
        let rc = unsafe {
            sys::cg_range_prove_batch(self.h, slot, ob.as_ptr(), ped_com.as_ptr(), rb.as_ptr(), n as u64, out.com_f.as_mut_ptr(),
                                      out.com_g.as_mut_ptr(), out.com_q.as_mut_ptr(), out.evals.as_mut_ptr(), out.proofs.as_mut_ptr(),
                                      out.pok_c.as_mut_ptr(), out.pok_s.as_mut_ptr(), out.challenges.as_mut_ptr(), out.status.as_mut_ptr())
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(out)
    }
}

/// What `GpuRangeKey::prove_batch` returns: the fields of n `RangeProof`s in the layouts `RangeProofRows` takes, the three
/// challenges (c_dleq, c, rho; n x 3 x 32 B) and one CG_SHOW_* byte per opening; a malformed opening has zero bytes throughout
pub struct RangeProofsMade {
    pub com_f: Vec<u8>,
    pub com_g: Vec<u8>,
    pub com_q: Vec<u8>,
    pub evals: Vec<u8>,
    pub proofs: Vec<u8>,
    pub pok_c: Vec<u8>,
    pub pok_s: Vec<u8>,
    pub challenges: Vec<u8>,
    pub status: Vec<u8>,
}

/// `DLogPoK`'s Merlin transcript for n showings of one shape (`cg_dlog_challenge_batch`, host only): `n_bases` per
/// statement, `bases` 64 B uncompressed each and shared by the batch, `k` n x n_statements x 32 B compressed, `y_head`
/// n x (n_statements - 1) x 64 B, `y_last` n x 64 B; one `context` for the batch.  Returns n x 32 B canonical challenges.
pub fn dlog_challenge_batch(context: Option<&[u8]>, n_bases: &[u32], bases: &[u8], k: &[u8], y_head: &[u8], y_last: &[u8]) -> Result<Vec<u8>, SynthesisError> {
    let n = y_last.len() / 64;
    let total: usize = n_bases.iter().map(|&b| b as usize).sum();
    if n_bases.is_empty() || y_last.len() != n * 64 || bases.len() != total * 64 || k.len() != n * n_bases.len() * 32 || y_head.len() != n * (n_bases.len() - 1) * 64 {
        return Err(SynthesisError::MalformedVerifyingKey);
    }
    let ctx = context.unwrap_or(&[]);
    let mut c = vec![0u8; n * 32];
    let rc = unsafe {
        sys::cg_dlog_challenge_batch(if ctx.is_empty() { std::ptr::null() } else { ctx.as_ptr() }, ctx.len() as u64, 0, n_bases.len() as u32,
                                     n_bases.as_ptr(), bases.as_ptr(), k.as_ptr(), y_head.as_ptr(), y_last.as_ptr(), n as u64, c.as_mut_ptr())
    };
    if rc != 0 {
        return Err(map_err(rc));
    }
    Ok(c)
}

/// The rows of `device_link_verify_batch`, n each, in the layouts of `cg_device_link_rows`
pub struct DeviceLinkRows {
    pub com1: Vec<u8>,
    pub comz: Vec<u8>,
    pub h_q: Vec<u8>,
    pub m: Vec<u8>,
    pub pi0_c: Vec<u8>,
    pub pi0_s: Vec<u8>,
    pub pi1_c: Vec<u8>,
    pub pi1_s: Vec<u8>,
}

/// The digests of `revealed_preimages` as `verify_show` places them among the public inputs (creds/src/lib.rs:590-603): per item
/// SHA-256 and the digest's first 31 bytes through `bits_to_num` (`cg_revealed_digest_batch`, host only).  Returns n x 32 B
/// canonical scalars.
pub fn revealed_digest_batch(items: &[&[u8]]) -> Result<Vec<u8>, SynthesisError> {
    let mut offsets = vec![0u64; items.len() + 1];
    let mut data = Vec::new();
    for (i, b) in items.iter().enumerate() {
        data.extend_from_slice(b);
        offsets[i + 1] = data.len() as u64;
    }
    let mut out = vec![0u8; items.len() * 32];
    let rc = unsafe { sys::cg_revealed_digest_batch(if data.is_empty() { std::ptr::null() } else { data.as_ptr() }, offsets.as_ptr(), items.len() as u64, out.as_mut_ptr()) };
    if rc != 0 {
        return Err(map_err(rc));
    }
    Ok(out)
}

impl Drop for GpuRangeKey {
    fn drop(&mut self) {
        unsafe { sys::cg_range_pk_free(self.h) }
    }
}

/// A `RangeProofVK` (creds/src/rangeproof.rs:74-78) resident on the GPU for verifying range proofs in batches
/// (`RangeProof::verify_n_bits`, rangeproof.rs:342-424) between the host's transcripts ("Verifying range proofs").
pub struct GpuRangeVerifyingKey {
    h: *mut sys::cg_range_vk,
}
unsafe impl Send for GpuRangeVerifyingKey {}
unsafe impl Sync for GpuRangeVerifyingKey {} // calls on one handle serialise inside the library

/// The flat arrays of `cg_range_verify_batch`, one row per proof, in the layouts the creation calls write
pub struct RangeProofRows<'a> {
    /// n x 64 B uncompressed each: the Pedersen commitment, then the proof's three commitments
    pub ped_com: &'a [u8],
    pub com_f: &'a [u8],
    pub com_g: &'a [u8],
    pub com_q: &'a [u8],
    /// n x 3 x 32 B (eval_g, eval_gw, eval_w_hat); n x 3 x 96 B (W uncompressed, then random_v; `None` as 0)
    pub evals: &'a [u8],
    pub proofs: &'a [u8],
    /// the range transcript's challenges, n each
    pub c: &'a [Fr],
    pub rho: &'a [Fr],
    /// n x (r_1, r_2): `KZG10::batch_check`'s randomizers, drawn by the caller
    pub randomizers: &'a [u128],
    /// dleq_proof.c, n; dleq_proof.s flattened, n x 6
    pub pok_c: &'a [Fr],
    pub pok_s: &'a [Fr],
}

impl GpuRangeVerifyingKey {
    /// `range_vk_bytes`: the 640 bytes of range_vk.bin; `n_bits`: 32 in the product
    pub fn load(range_vk_bytes: &[u8], n_bits: u32) -> Result<Self, SynthesisError> {
        let mut h = std::ptr::null_mut();
        let rc = unsafe { sys::cg_range_vk_load(&mut h, range_vk_bytes.as_ptr(), range_vk_bytes.len() as u64, n_bits, -1) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(GpuRangeVerifyingKey { h })
    }

    /// Registers the Pedersen bases of one range-checked input (groth16rand.rs:319-323) and returns their slot.
    pub fn add_bases(&self, gamma_abc_point: &G1Affine, delta_g1: &G1Affine) -> Result<u32, SynthesisError> {
        let mut b = Vec::with_capacity(128);
        for p in [gamma_abc_point, delta_g1] {
            p.serialize_uncompressed(&mut b).map_err(|_| SynthesisError::AssignmentMissing)?;
        }
        let mut slot = 0u32;
        let rc = unsafe { sys::cg_range_vk_add_bases(self.h, b.as_ptr(), &mut slot) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(slot)
    }

    /// As `GpuVerifyingKey::set_latency_mode`, for the pairing of `verify_batch` (`cg_range_vk_set_latency_mode`)
    pub fn set_latency_mode(&self, on: bool) -> Result<(), SynthesisError> {
        let rc = unsafe { sys::cg_range_vk_set_latency_mode(self.h, on as i32) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(())
    }

    /// (group stage, pairing) HIP-event milliseconds of the last call
    pub fn last_kernel_ms(&self) -> Result<(f32, f32), SynthesisError> {
        let (mut a, mut b) = (0f32, 0f32);
        let rc = unsafe { sys::cg_range_vk_last_kernel_ms(self.h, &mut a, &mut b) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((a, b))
    }

    /// Returns (verdicts: n x CG_VERIFY_*, k: n x 2 x 32 B compressed k_0, k_1).  A proof is valid when its verdict is
    /// CG_VERIFY_ACCEPT and the DLEQ transcript over the bases, k and y (dlog.rs:130-174) gives back its pok_c.
    pub fn verify_batch(&self, slot: u32, rows: &RangeProofRows) -> Result<(Vec<u8>, Vec<u8>), SynthesisError> {
        let n = rows.c.len();
        if rows.ped_com.len() != n * 64 || rows.com_f.len() != n * 64 || rows.com_g.len() != n * 64 || rows.com_q.len() != n * 64
            || rows.evals.len() != n * 96 || rows.proofs.len() != n * 288 || rows.rho.len() != n || rows.randomizers.len() != 2 * n
            || rows.pok_c.len() != n || rows.pok_s.len() != n * sys::CG_RANGE_N_RESP
        {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let (cb, hb, pc, ps) = (canonical_bytes(rows.c), canonical_bytes(rows.rho), canonical_bytes(rows.pok_c), canonical_bytes(rows.pok_s));
        let zb: Vec<u8> = rows.randomizers.iter().flat_map(|r| r.to_le_bytes()).collect();
        let (mut verdicts, mut k) = (vec![0u8; n], vec![0u8; n * 64]);
        let rc = unsafe {
            sys::cg_range_verify_batch(self.h, slot, rows.ped_com.as_ptr(), rows.com_f.as_ptr(), rows.com_g.as_ptr(), rows.com_q.as_ptr(),
                                       rows.evals.as_ptr(), rows.proofs.as_ptr(), cb.as_ptr(), hb.as_ptr(), zb.as_ptr(), pc.as_ptr(),
                                       ps.as_ptr(), n as u64, verdicts.as_mut_ptr(), k.as_mut_ptr())
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((verdicts, k))
    }

    /// `RangeProof::verify_n_bits` in one call (`cg_range_verify_proofs_batch`): c and rho are derived and the DLEQ's
    /// challenge is recomputed and compared on the GPU, so `rows.c` and `rows.rho` are not read (pass empty slices).
    /// CG_VERIFY_ACCEPT exactly where `verify_n_bits` returns true.
    pub fn verify_proofs_batch(&self, slot: u32, rows: &RangeProofRows) -> Result<Vec<u8>, SynthesisError> {
        let n = rows.pok_c.len();
        if rows.ped_com.len() != n * 64 || rows.com_f.len() != n * 64 || rows.com_g.len() != n * 64 || rows.com_q.len() != n * 64
            || rows.evals.len() != n * 96 || rows.proofs.len() != n * 288 || rows.randomizers.len() != 2 * n
            || rows.pok_s.len() != n * sys::CG_RANGE_N_RESP
        {
            return Err(SynthesisError::MalformedVerifyingKey);
        }
        let (pc, ps) = (canonical_bytes(rows.pok_c), canonical_bytes(rows.pok_s));
        let zb: Vec<u8> = rows.randomizers.iter().flat_map(|r| r.to_le_bytes()).collect();
        let mut verdicts = vec![0u8; n];
        let rc = unsafe {
            sys::cg_range_verify_proofs_batch(self.h, slot, rows.ped_com.as_ptr(), rows.com_f.as_ptr(), rows.com_g.as_ptr(), rows.com_q.as_ptr(),
                                              rows.evals.as_ptr(), rows.proofs.as_ptr(), zb.as_ptr(), pc.as_ptr(), ps.as_ptr(), n as u64,
                                              verdicts.as_mut_ptr())
        };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(verdicts)
    }
}

impl Drop for GpuRangeVerifyingKey {
    fn drop(&mut self) {
        unsafe { sys::cg_range_vk_free(self.h) }
    }
}

/// `MultiCommitGens { G, h }` of spartan_t256 (forks/Spartan-t256/src/commitments.rs) resident on the GPU as fixed-base
/// tables (`cg_t256_gens_load`), and on it the commitments of pi2's witness.  Points are uncompressed, x ‖ y big-endian;
/// scalars 32 B little-endian; commitments come back compressed, 33 B.  These byte forms are UNVERIFIED readings of
/// halo2curves (include/crescent_gpu.h): a caller converts with halo2curves' own `to_bytes` / `from_bytes` and compares once.
pub struct GpuT256Gens {
    h: *mut sys::cg_t256_gens,
    n_gens: usize,
}
unsafe impl Send for GpuT256Gens {}
unsafe impl Sync for GpuT256Gens {} // calls on one handle serialise inside the library

impl GpuT256Gens {
    /// `g_xy`: n_gens x 64 B, `h_xy`: 64 B.  `MultiCommitGens::new` itself stays on the host, which has the points.
    pub fn load(g_xy: &[u8], h_xy: &[u8]) -> Result<Self, SynthesisError> {
        if g_xy.len() % 64 != 0 || h_xy.len() != 64 {
            return Err(SynthesisError::AssignmentMissing);
        }
        let mut h = std::ptr::null_mut();
        let rc = unsafe { sys::cg_t256_gens_load(g_xy.as_ptr(), (g_xy.len() / 64) as u64, h_xy.as_ptr(), &mut h) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok(GpuT256Gens { h, n_gens: g_xy.len() / 64 })
    }

    /// (n_gens, bytes of the set's tables on the device) (`cg_t256_gens_info`)
    pub fn info(&self) -> Result<(u64, u64), SynthesisError> {
        let (mut n, mut b) = (0u64, 0u64);
        let rc = unsafe { sys::cg_t256_gens_info(self.h, &mut n, &mut b) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((n, b))
    }

    /// `Vec<Scalar>::commit` (commitments.rs:88-99) for n rows (`cg_t256_commit_rows_batch`): `scalars` n x n_gens x 32 B,
    /// `blinds` n x 32 B.  Returns (n x 33 B, n status bytes: CG_SHOW_MADE, or CG_SHOW_MALFORMED and zero bytes for a row with
    /// a scalar or blind >= q).  With n_gens = 1 this is `Scalar::commit`.
    pub fn commit_rows_batch(&self, scalars: &[u8], blinds: &[u8]) -> Result<(Vec<u8>, Vec<u8>), SynthesisError> {
        if blinds.len() % 32 != 0 || scalars.len() != blinds.len() * self.n_gens {
            return Err(SynthesisError::AssignmentMissing);
        }
        let n = blinds.len() / 32;
        let (mut out, mut status) = (vec![0u8; 33 * n], vec![0u8; n]);
        let rc = unsafe { sys::cg_t256_commit_rows_batch(self.h, scalars.as_ptr(), blinds.as_ptr(), n as u64, out.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((out, status))
    }

    /// `DensePolynomial::commit` (dense_mlpoly.rs:181-206) for n proofs (`cg_hyrax_commit_batch`): `vars` n x 2^num_vars x 32 B,
    /// `blinds` n x L x 32 B with L = 2^(num_vars / 2).  Returns (n x L x 33 B in `PolyCommitment.C`'s order, n status bytes,
    /// one per proof).
    pub fn hyrax_commit_batch(&self, num_vars: u32, vars: &[u8], blinds: &[u8]) -> Result<(Vec<u8>, Vec<u8>), SynthesisError> {
        if num_vars >= 63 {
            return Err(SynthesisError::AssignmentMissing);
        }
        let l = 1usize << (num_vars / 2);
        if blinds.len() % (32 * l) != 0 || vars.len() != (blinds.len() / l) << num_vars {
            return Err(SynthesisError::AssignmentMissing);
        }
        let n = blinds.len() / (32 * l);
        let (mut out, mut status) = (vec![0u8; 33 * l * n], vec![0u8; n]);
        let rc = unsafe { sys::cg_hyrax_commit_batch(self.h, num_vars, vars.as_ptr(), blinds.as_ptr(), n as u64, out.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((out, status))
    }

    /// (`cg_t256_commit_last_kernel_ms`) HIP-event milliseconds of the last call - the check, the group stage (the rows' sums
    /// and their normalisation) - and how many lanes shared a row in its last chunk
    pub fn commit_last_kernel_ms(&self) -> Result<([f32; 2], u32), SynthesisError> {
        let (mut ms, mut lanes) = ([0f32; 2], 0u32);
        let rc = unsafe { sys::cg_t256_commit_last_kernel_ms(self.h, ms.as_mut_ptr(), &mut lanes) };
        if rc != 0 {
            return Err(map_err(rc));
        }
        Ok((ms, lanes))
    }
}

impl Drop for GpuT256Gens {
    fn drop(&mut self) {
        unsafe { sys::cg_t256_gens_free(self.h) }
    }
}
