/*
 * crescent_gpu.h — C ABI of the MI355X-native Groth16 prover hot path for Crescent.
 *
 * This is the drop-in boundary for `forks/groth16` of microsoft/crescent-credentials: every entry
 * point names the reference interface it replaces (paths relative to the reference root).  The
 * reference has no FFI today (Rust generics only); the seams are
 *   - the `QAP: R1CSToQAP` type parameter      forks/groth16/src/lib.rs:55, r1cs_to_qap.rs:49-98
 *   - the three `msm_bigint` call sites         forks/groth16/src/prover.rs:66,74,266
 *   - the caller                                creds/src/lib.rs:283 (Groth16::<Bn254>::prove)
 * INTEGRATION.md shows the Rust `extern "C"` block + shim a maintainer would add.
 *
 * Conventions
 *   - All field elements cross the boundary as 32-byte little-endian integers.
 *     CG_FORM_CANONICAL : the plain integer in [0, p)   (what ark-serialize files contain and what
 *                         `into_bigint()` yields, prover.rs:64,71,86)
 *     CG_FORM_MONTGOMERY: x * 2^256 mod p, i.e. arkworks' in-memory Fp256<MontBackend<_,4>> limbs
 *                         (KAT: forks/circom-compat/src/zkey.rs:397-402)
 *   - G1 affine point  = x ‖ y                  (64 bytes);   identity = 64 zero bytes
 *   - G2 affine point  = x.c0 ‖ x.c1 ‖ y.c0 ‖ y.c1 (128 bytes); identity = 128 zero bytes
 *     (same component order as snarkjs/arkworks, zkey.rs:421-431)
 *   - Scalars are CG_FORM_CANONICAL, with ONE exception a host opts into: on a handle loaded with
 *     CG_FLAG_SCALARS_MONTGOMERY (cg_circuit_load, cg_msm_load_g1/g2) or cg_qap_load_form(.., CG_FORM_MONTGOMERY) every
 *     ASSIGNMENT a call receives - full_assignment / d_full_assignment of cg_prove, cg_prove_dev, cg_check_witness,
 *     cg_prove_partial, cg_prove_partial_q, cg_prove_partial_q_begin, cg_witness_map, cg_witness_map_coset,
 *     cg_witness_map_coset_half, cg_qap_witness_map, cg_qap_check_witness; `scalars` of cg_msm_run - is
 *     CG_FORM_MONTGOMERY, i.e. a `Vec<Fr>` as it lies in memory, and the coefficients cg_witness_map /
 *     cg_qap_witness_map return are in the same form.  The GPU converts (one pass over the vector; a device-resident
 *     assignment is read, never written).  A Montgomery element >= r is not a field element: CG_ERR_INVALID_ARGUMENT,
 *     nothing written, exactly as for a non-canonical element.  Canonical on every handle: the single scalars r, s;
 *     the a/b/c of cg_witness_report; the vectors no host computes with and only passes from shard to shard (q_out,
 *     q_slice, a_slice, b_slice, the _half outputs); proofs and partial records.  cg_scalars_convert changes a vector's
 *     form on the host.
 *   - Every function returns CG_OK (0) or a negative cg_status; cg_last_error() returns a
 *     thread-local human-readable message for the last failure on the calling thread.
 *   - The caller owns every host buffer; the library copies what it keeps.
 *   - A cg_ctx is bound to one GPU.  Calls on different contexts are independent and may run
 *     concurrently from different threads; calls on one context take one of its `proof_slots`
 *     working sets each (blocking while none is free), so up to that many proofs overlap on the GPU.
 */
#ifndef CRESCENT_GPU_H
#define CRESCENT_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum cg_status {
    CG_OK = 0,
    CG_ERR_INVALID_ARGUMENT = -1,
    CG_ERR_NO_DEVICE = -2,            /* no HIP device / HIP runtime failure at init */
    CG_ERR_HIP = -3,                  /* a HIP call failed; see cg_last_error() */
    CG_ERR_OUT_OF_MEMORY = -4,
    CG_ERR_POLY_DEGREE_TOO_LARGE = -5, /* SynthesisError::PolynomialDegreeTooLarge, r1cs_to_qap.rs:156-157 */
    CG_ERR_MALFORMED_KEY = -6,        /* query lengths inconsistent with the circuit (SynthesisError::MalformedVerifyingKey analogue) */
    CG_ERR_PARSE = -7,                /* .r1cs / serialized key parse failure */
    CG_ERR_UNSATISFIED = -8           /* witness does not satisfy the R1CS (cg_check_witness, CG_FLAG_CHECK_WITNESS) */
} cg_status;

enum { CG_FORM_CANONICAL = 0, CG_FORM_MONTGOMERY = 1 };

typedef struct cg_ctx cg_ctx;

/* Packed arrays of a Groth16 proving key.
 * Replaces: `ProvingKey<E>` / `VerifyingKey<E>` operands of the prover,
 *           forks/groth16/src/data_structures.rs:31-44,101-118.
 * Lengths must be (generator.rs:140,162,168,174-179,185):
 *   a_query, b_g1_query, b_g2_query : num_variables
 *   l_query                         : num_variables - num_inputs
 *   h_query                         : domain_size - 1   (domain_size = next pow2 >= m + num_inputs) */
typedef struct cg_proving_key {
    uint32_t coord_form;        /* CG_FORM_CANONICAL or CG_FORM_MONTGOMERY for every coordinate below */
    const uint8_t* alpha_g1;    /* vk.alpha_g1  64 B */
    const uint8_t* beta_g1;     /* pk.beta_g1   64 B */
    const uint8_t* delta_g1;    /* pk.delta_g1  64 B */
    const uint8_t* beta_g2;     /* vk.beta_g2  128 B */
    const uint8_t* delta_g2;    /* vk.delta_g2 128 B */
    const uint8_t* a_query;     uint64_t a_len;      /* G1 */
    const uint8_t* b_g1_query;  uint64_t b_g1_len;   /* G1 */
    const uint8_t* b_g2_query;  uint64_t b_g2_len;   /* G2 */
    const uint8_t* h_query;     uint64_t h_len;      /* G1 */
    const uint8_t* l_query;     uint64_t l_len;      /* G1 */
} cg_proving_key;

/* One R1CS matrix in CSR form.
 * Replaces: one of `ConstraintMatrices<F>::{a,b,c}` (Vec<Vec<(F, usize)>>),
 *           operand of forks/groth16/src/prover.rs:26-33 / r1cs_to_qap.rs:150-155.
 * Row i holds terms [row_ptr[i], row_ptr[i+1]); column = variable index (instance vars first,
 * forks/circom-compat/src/circom/circuit.rs:61-67). */
typedef struct cg_csr {
    const uint64_t* row_ptr;   /* num_constraints + 1 entries */
    const uint32_t* col;       /* nnz entries, each < num_variables */
    const uint8_t* coeff;      /* nnz x 32 B, CG_FORM_CANONICAL */
    uint64_t nnz;
} cg_csr;

typedef struct cg_options {
    int32_t device;        /* HIP device ordinal; -1 = current device */
    int32_t window_bits;   /* Pippenger window c; 0 = library default for the size */
    int32_t shard_rank;    /* multi-GPU MSM range sharding: this context's rank ... */
    int32_t shard_count;   /* ... of shard_count; 0 or 1 = unsharded.  A shard with proof_slots > 1 keeps that many
                              sharded proofs in flight (cg_prove_partial from as many threads) */
    int32_t proof_slots;   /* proofs that may be in flight on this context at once (each has its own working
                              set and streams; cg_prove* from different threads overlap on the GPU); 0 = 1, at
                              most 16.  1 = a latency context (five streams per proof); more = a throughput
                              context (one stream per proof; twelve reach the full rate at the rs256 size) */
    int32_t flags;         /* CG_FLAG_* (the library reads none of ITS OWN switches from the environment: what a host may choose is here) */
    int32_t hw_queues;     /* the hardware queues the host's HIP runtime maps its streams onto (the runtime's own GPU_MAX_HW_QUEUES,
                              read once when HIP initialises; default 4), if the host knows; 0 = the library looks at that variable:
                              cg_init sets it to 20 when the host has not - which only takes effect if HIP was not initialised before
                              cg_init - and a throughput context then shares four copy-only streams among its upload buffers.  A host that
                              initialises HIP first and cannot export the variable passes the real count here (4 unless it chose
                              otherwise): with fewer queues than proof_slots + 4 every upload buffer keeps a stream of its own */
    int32_t shard_span;    /* sharded contexts: 0 = this shard owns the shard_rank-th of shard_count EQUAL parts of every query.
                              Otherwise lo | hi << 16, both in 1/10000 of a query's length (0 <= lo < hi <= 10000): the shard owns the
                              entries [n·lo/10000, n·hi/10000) of each of the five queries (of the h query: that contiguous range
                              of its coset points).  The spans of a proof's shards must tile [0, 10000] - the host's business, as
                              the ranks are.  For hosts that give unequal shares: the ranks that also run (half of) the witness map
                              take a smaller share of the MSMs.  cg_h_scalars_slice then answers for the
                              context's own shard only */
} cg_options;

/* By default cg_circuit_load moves the h query into the evaluation basis of the coset and folds the C matrix into
 * the l query (two inverse DFTs over the h query's G1 points, ~1.6 s at 2^21), so that a proof needs four transforms
 * instead of seven and no sparse product with C: Σ h_i·H_i of prover.rs:63-66 is computed as Σ q_j·H'_j over the coset
 * values q_j = a·b/Z plus a per-wire term carried by the l query — the same group elements, hence the same proof bytes
 * for any assignment.  This flag keeps both queries as loaded and runs the reference's seven transforms
 * (r1cs_to_qap.rs:179-210) per proof. */
enum {
    CG_FLAG_H_COEFFICIENT_BASIS = 1,
    /* How a context arranges a proof's work on the GPU.  By default proof_slots decides: one slot = a LATENCY context (the
     * five MSMs and the witness map on five streams, short accumulation segments, tree reductions, callers spin while
     * they wait), several = a THROUGHPUT context (one stream per proof, long segments, fewest instructions, callers
     * sleep-poll).  A host may force either - e.g. throughput kernels for a single slot that shares the GPU with other
     * contexts, or the latency arrangement for two slots.  Both set = CG_ERR_INVALID_ARGUMENT. */
    CG_FLAG_LATENCY_MODE = 2,
    CG_FLAG_THROUGHPUT_MODE = 4,
    /* Calling threads spin in the HIP runtime while they wait for their proof instead of sleep-polling (a throughput
     * context's default): lowest wake-up latency, one busy CPU per proof in flight. */
    CG_FLAG_SPIN_WAIT = 8,
    /* Sharded contexts (shard_count a power of two): own a contiguous range of the h query's coset points instead of
     * the points j = shard_rank (mod shard_count); the shard then runs four full-size transforms per proof. */
    CG_FLAG_CONTIGUOUS_H_SHARDS = 16,
    /* Sharded contexts over a folded key (SURVEY 8e's other arrangement: "run the witness map on GPU 0 and scatter h"): this
     * shard never runs the witness map - its h scalars arrive with every proof (cg_prove_partial_q), computed once for all
     * shards by cg_witness_map_coset on a context loaded WITHOUT this flag.  The context then holds no witness-map vectors
     * and no matrices; cg_prove_partial / cg_witness_map on it are CG_ERR_INVALID_ARGUMENT. */
    CG_FLAG_H_SCALARS_EXTERNAL = 32,
    /* Staged load: cg_circuit_load returns as soon as the context can PROVE, and finishes loading behind the first proofs.
     * The reference's caller reads its two files and proves once (`create_client_state`, creds/src/lib.rs:255-301; the sample
     * client does so per credential, sample/client_helper/src/main.rs:177-216), so what it waits for is load + ONE proof, and
     * two thirds of a synchronous load are spent on tables that only pay off over many proofs (the change of basis of the
     * h query, ~1.5 s at 2^21, and the per-window tables, ~0.6 s).  With this flag the load copies the key and the matrices,
     * keeps every query as its row-0 table and returns; proofs then run in the WARM-UP arrangement - the reference's own
     * (seven transforms, plain h query, r1cs_to_qap.rs:179-210) over classic Pippenger with one bucket set per window - while
     * a worker thread of the library builds the final arrangement (folded key, per-window tables, windows chosen from the
     * first finished proof's digit statistics when there is one) and swaps it in between two proofs.  Proof bytes are the
     * same in both arrangements (they are the same group elements).  cg_ctx_wait_ready blocks until the swap; a host that
     * never calls it loses nothing but the first seconds' throughput.  Honoured for unsharded contexts over the folded key;
     * sharded contexts and CG_FLAG_H_COEFFICIENT_BASIS load synchronously as before. */
    CG_FLAG_STAGED_LOAD = 64,
    /* A THROUGHPUT context with more than one slot holds up to two slots more than proof_slots: the LONE slots, arranged as a
     * latency context's (five streams, short segments).  A proof that arrives when fewer than two proofs of the context are in
     * flight - a server between requests: the sample client proves one credential per task,
     * sample/client_helper/src/main.rs:177-216 - runs on one of them (at 2^21 from pageable memory: 7.7 ms instead of 10.9 alone,
     * 13.8 instead of 15.3-16.4 in a pair); proofs that find more in flight take the one-stream slots as before, so the steady
     * rate is untouched.  Costs a latency slot's memory each (cg_ctx_info.lone_slot_bytes is their sum; a device without room
     * for them does without) and no stream: they run on streams of the last one-stream slots.  A call that asks for cg_timings
     * always runs on a one-stream slot: its phases are then stand-alone durations that add up.  This flag leaves them out. */
    CG_FLAG_NO_LONE_SLOT = 128,
    /* Check every witness before it is proved (off by default, as the reference's check is a debug assertion in release
     * builds: forks/groth16/src/prover.rs:197).  Every call that runs the sparse products on this context - cg_prove,
     * cg_prove_dev, cg_prove_partial, cg_prove_partial_q_begin + cg_partial_witness_map_coset, cg_witness_map,
     * cg_witness_map_coset - also forms C·w (over the folded key that is the third product it otherwise skips) and queues
     * cg_check_witness's kernel between the products and the first transform.  A witness that fails a constraint: the call
     * returns CG_ERR_UNSATISFIED (cg_last_error names the first failing constraint and their number), writes nothing to
     * proof_out / out_partials (the output vector of a witness-map call is then unspecified), and gives its slot back as
     * after any other failure.  The verdict is
     * read after the synchronisation the call makes anyway.  NOT checked: the _q forms (cg_prove_partial_q, _q_finish,
     * _q_finish2), whose h scalars come from outside, and the _half forms, which see one matrix only.
     * With CG_FLAG_H_SCALARS_EXTERNAL (no matrices on the context) the load is CG_ERR_INVALID_ARGUMENT. */
    CG_FLAG_CHECK_WITNESS = 256,
    /* Assignments in arkworks' in-memory form (Conventions): every assignment a call on this context receives is
     * x·2^256 mod r, 32 little-endian bytes per element - `Fr.0`, so a Rust host copies its `Vec<Fr>` as it is instead of
     * running `into_bigint()` over it - and cg_witness_map returns its coefficients in that form.  The context converts on
     * the GPU: a host assignment in place in its upload buffer, behind the copy; a device-resident one (cg_prove_dev, ..)
     * from the caller's buffer, which is not written, into an upload buffer.  An element >= r is refused as a
     * non-canonical one is on other contexts.  Combines with every other flag; also honoured by cg_msm_load_g1/g2 (the
     * `scalars` of cg_msm_run).  cg_timings of such a context: upload_ms stays the copy alone; the pass is part of
     * total_ms and is reported on its own in reserved_ms (0 on every other context). */
    CG_FLAG_SCALARS_MONTGOMERY = 512
};

/* Per-phase wall/GPU times of one cg_prove call, mirroring the reference's `print-trace` phases
 * (forks/groth16/src/prover.rs:35-36,62,93,103,115,123). Milliseconds. */
typedef struct cg_timings {
    float upload_ms;       /* host -> device copy of the assignment (0 for *_dev entry points) */
    float witness_map_ms;  /* "R1CS to QAP witness map" */
    float msm_h_ms;        /* "Compute C": h_query MSM.  A throughput context reduces the buckets of its four G1 MSMs in ONE
                            * batched chain behind the h MSM, the last on the proof's stream: that chain's time is counted
                            * here, and msm_l_ms, msm_a_ms, msm_b1_ms then end with the MSM's last combine level */
    float msm_l_ms;        /* "Compute C": l_query MSM */
    float msm_a_ms;        /* "Compute A" */
    float msm_b1_ms;       /* "Compute B in G1" */
    float msm_b2_ms;       /* "Compute B in G2" */
    float finish_ms;       /* "Finish C" + affine normalisation + serialisation (host) */
    float total_ms;        /* "Groth16::Prover" */
    uint64_t msm_g1_pairs; /* (base, scalar) pairs consumed by the four G1 MSMs */
    uint64_t msm_g2_pairs;
    /* HIP-event durations of the dominant kernels, summed over this proof's launches */
    float accum_g1_ms;     /* bucket-accumulation kernel (k_accum_affine<Fq>), the four G1 MSMs */
    float accum_g2_ms;     /* same kernel over Fq2 (the G2 MSM) */
    float sort_ms;         /* grouping the digit entries by bucket (counting partition), all five MSMs */
    float reserved_ms;     /* CG_FLAG_SCALARS_MONTGOMERY contexts: the Montgomery -> canonical pass over the assignment; else 0 */
    uint64_t entries_g1;   /* non-zero signed digits (= mixed additions) accumulated, G1 */
    uint64_t entries_g2;
    uint32_t accum_g1_launches;
    uint32_t accum_g2_launches;
} cg_timings;

/* Process-wide initialisation: checks that a HIP device is present.
 * n_devices/device_ids may be 0/NULL (use whatever is visible). */
int cg_init(int n_devices, const int* device_ids);

/* The GPU that entry points WITHOUT a device of their own run on when called from this thread afterwards: cg_setup,
 * cg_msm_g1/g2, cg_ntt, cg_fixed_base_*, and the loaders given device -1.  (Contexts carry their device and switch to
 * it on every call.)  A host with one process per GPU calls this once with its local rank; the reference has no
 * counterpart (it has no devices). */
int cg_set_device(int32_t device);

/* Thread-local description of the last error on this thread ("" if none). */
const char* cg_last_error(void);

/* Load a circuit: copy the proving key and the three constraint matrices to the GPU, build the
 * per-window base tables and the NTT tables.  One-time per circuit.
 * Replaces: `read_from_file::<ProverParams>` + `CircomConfig::new` products as consumed by the
 *           prover (creds/src/lib.rs:258,268), and `cs.to_matrices()` (r1cs_to_qap.rs:62).
 * num_inputs (ℓ) counts the constant-one variable; num_variables (M) = instance + witness. */
int cg_circuit_load(cg_ctx** out, const cg_proving_key* pk, const cg_csr abc[3],
                    uint64_t num_inputs, uint64_t num_constraints, uint64_t num_variables,
                    const cg_options* opt);

/* Waits for every call that is still inside the context (cg_prove*, cg_prove_partial, cg_assemble, cg_witness_map: their GPU
 * work AND their host tails) and then frees it.  No call may START on the context once this one has. */
void cg_circuit_free(cg_ctx* ctx);

/* Create one Groth16 proof.
 * Replaces: `Groth16::<E,QAP>::create_proof_with_reduction_and_matrices`,
 *           forks/groth16/src/prover.rs:26-51 (and through it :54-136, :256-274 and
 *           r1cs_to_qap.rs:150-213).
 * full_assignment: num_variables x 32 B canonical - Montgomery on a CG_FLAG_SCALARS_MONTGOMERY context, here and in every
 *       entry point below that takes one - (instance ‖ witness, full_assignment[0] = 1).
 * r, s: 32 B canonical each (prover.rs:150-151 samples them; r = s = 0 gives the no-zk proof,
 *       prover.rs:160-173).
 * proof_out: 256 B = ark-serialize uncompressed a ‖ b ‖ c (data_structures.rs:7-14).
 * timings may be NULL.
 * A failed one-time window re-tune never fails the proof it follows; if it ran out of device memory while the proof
 * slots were being re-sized, every LATER proof on the context returns CG_ERR_OUT_OF_MEMORY (free and reload). */
int cg_prove(cg_ctx* ctx, const uint8_t* full_assignment, const uint8_t r[32], const uint8_t s[32],
             uint8_t proof_out[256], cg_timings* timings);

/* Same, with the assignment already resident in this context's GPU memory
 * (d_full_assignment is a device pointer, num_variables x 32 B canonical). */
int cg_prove_dev(cg_ctx* ctx, const void* d_full_assignment, const uint8_t r[32], const uint8_t s[32],
                 uint8_t proof_out[256], cg_timings* timings);

/* Does this assignment satisfy the R1CS, and if not, which constraint fails first?
 * Replaces: `cs.is_satisfied()` / `cs.which_is_unsatisfied()` in the circom builder
 *           (forks/circom-compat/src/circom/builder.rs:82-94) and `debug_assert!(cs.is_satisfied())`
 *           (forks/groth16/src/prover.rs:197): <A_i,w>·<B_i,w> = <C_i,w> for every constraint i < num_constraints.
 * The three sparse products and one pass over their results on the GPU; takes one of the context's proof slots like a
 * proof, so it may be called from any thread next to proofs in flight.  Works on whole and sharded contexts, over both
 * key layouts, and in both phases of a staged load.
 * Returns CG_OK (satisfied; report->n_unsatisfied = 0), CG_ERR_UNSATISFIED (report filled; cg_last_error says
 * "constraint <i> of <m> is not satisfied (<n> in all)"), CG_ERR_INVALID_ARGUMENT for an assignment element >= the
 * scalar field modulus (as cg_prove) and on a CG_FLAG_H_SCALARS_EXTERNAL context (it holds no matrices).
 * report may be NULL. */
typedef struct cg_witness_report {
    uint64_t n_unsatisfied;      /* constraints with <A_i,w>·<B_i,w> != <C_i,w>; 0 = satisfied */
    uint64_t first_unsatisfied;  /* smallest such i (what which_is_unsatisfied names); undefined when n_unsatisfied == 0 */
    uint8_t  a[32];              /* <A_i,w> of that row, 32-byte little-endian canonical */
    uint8_t  b[32];              /* <B_i,w> */
    uint8_t  c[32];              /* <C_i,w> */
    float    check_ms;           /* HIP-event time of the products + the check */
    int32_t  reserved[7];
} cg_witness_report;
int cg_check_witness(cg_ctx* ctx, const void* full_assignment, int assignment_on_device, cg_witness_report* report);

/* Page-locked host memory for assignments.
 * Replaces: the allocation behind `full_assignment: &[E::ScalarField]` (forks/groth16/src/prover.rs:33; built as
 *           `[instance_assignment, witness_assignment].concat()` at r1cs_to_qap.rs:68-72 from what the WASM witness
 *           calculator returned, forks/circom-compat/src/circom/builder.rs:71-98).  cg_prove accepts ANY
 *           host pointer; from pageable memory the 32·num_variables-byte upload is staged by the HIP runtime inside the call,
 *           from page-locked memory it is one asynchronous DMA that overlaps the other proofs in flight.  A host that
 *           can choose where the witness calculator writes its output takes the buffer from cg_host_alloc; a host that
 *           cannot may pin its own buffer once with cg_host_register (and must cg_host_unregister it before freeing it).
 * cg_host_alloc returns NULL on failure (cg_last_error says why). */
void* cg_host_alloc(uint64_t bytes);
void cg_host_free(void* p);
int cg_host_register(void* p, uint64_t bytes);
int cg_host_unregister(void* p);

/* What a loaded circuit occupies and how its MSMs are configured.  The reference's prover has no counterpart (its key is
 * a Vec in host memory, data_structures.rs:101-118); a host sizing `proof_slots`, or running several circuits on one GPU,
 * needs the numbers, and a host that relies on the one-time window re-tune (see cg_options.window_bits) needs to know
 * whether it happened. */
typedef struct cg_ctx_info {
    uint64_t table_bytes;        /* per-window base tables of the five queries + validity flags (shared by all slots) */
    uint64_t matrix_bytes;       /* resident constraint matrices + NTT / coset tables */
    uint64_t slot_bytes;         /* ONE proof slot's working set; the context holds proof_slots of them */
    uint64_t total_bytes;        /* table_bytes + matrix_bytes + proof_slots x slot_bytes + lone_slot_bytes */
    uint64_t device_free_bytes;  /* hipMemGetInfo at the time of the call */
    uint64_t device_total_bytes;
    int32_t proof_slots;
    int32_t window_bits[5];      /* current window of the h, l, a, b_g1, b_g2 MSMs */
    int32_t tuned;               /* 1 once the assignment-driven windows were re-chosen from a proof's digit statistics */
    int32_t retune_skipped_for_memory; /* queries whose re-tuned table did not fit beside the old one: they keep the size-based window */
    int32_t retune_attempts;     /* proofs inspected for the re-tune so far (it gives up after a few degenerate ones) */
    int32_t shard_rank;
    int32_t shard_count;
    int32_t latency_mode;        /* 1: short accumulation segments + tree reductions (one proof at a time); 0: throughput */
    int32_t warmup;              /* 1: a staged load (CG_FLAG_STAGED_LOAD) whose final arrangement is not in force yet */
    int32_t lone_slots;          /* extra slots for proofs that arrive (nearly) alone: 0-2 (CG_FLAG_NO_LONE_SLOT) */
    int32_t reserved[2];
    /* slot_bytes by kind (they add up to it).  In a throughput context the five MSMs of a proof run one after another and
     * share one set of entry lists and segment pieces, sized for the largest of them; a latency context (proof_slots = 1)
     * runs them concurrently and holds a set per MSM. */
    uint64_t slot_entry_bytes;     /* digit-entry lists: 8 B x bases x windows, two of them (grouped by the high / by the whole key) */
    uint64_t slot_piece_bytes;     /* first / last run of every accumulation segment, for the wave-combine levels */
    uint64_t slot_bucket_bytes;    /* bucket arrays, row / column sums of the reduction, partition histograms and cursors */
    uint64_t slot_transform_bytes; /* the witness map's vectors (assignment + four domain-sized vectors) and the h MSM's scalars */
    uint64_t slot_upload_bytes;    /* one device copy of an assignment arriving from the host (the context holds proof_slots + 2) */
    uint64_t lone_slot_bytes;      /* the lone slots' working sets together (each a set of entry lists and pieces per MSM) */
} cg_ctx_info;
int cg_ctx_get_info(cg_ctx* ctx, cg_ctx_info* out);

/* Where the time of cg_circuit_load went, by the reference's own timer names where it has them ("Reading ProverParams",
 * "Reading R1CS", creds/src/lib.rs:257,266 - there the cost is deserialisation; here it is the copy into HBM and the tables).
 * Milliseconds on the host clock.  With CG_FLAG_STAGED_LOAD, fold_ms / window_tables_ms / final_slots_ms belong to the
 * background part and are 0 until it is done (ready = 1). */
typedef struct cg_load_timings {
    float total_ms;           /* cg_circuit_load, call to return */
    float matrices_ms;        /* the three matrices: validation, coefficient dictionary, sliced layout, copy (host threads) */
    float domain_ms;          /* twiddle and coset tables of the evaluation domain */
    float key_copy_ms;        /* the five queries: host -> device copy, Montgomery import, row-0 table points */
    float fold_ms;            /* h query -> coset evaluation basis, C matrix folded into the l query (two DFTs over G1) */
    float window_tables_ms;   /* rows 1.. of the per-window tables of the five queries */
    float slots_ms;           /* proof slots and upload buffers (the warm-up slots of a staged load) */
    float final_slots_ms;     /* staged load: the proof slots of the final arrangement */
    float background_ms;      /* staged load: the worker's whole run, return of cg_circuit_load -> swap done */
    float swap_wait_ms;       /* staged load: how long the swap waited for the proofs in flight to drain */
    float ready_after_ms;     /* staged load: call of cg_circuit_load -> final arrangement in force */
    int32_t staged;           /* 1: the load was staged */
    int32_t ready;            /* 1: the final arrangement is in force (always 1 for a synchronous load) */
    int32_t windows_from_proof; /* staged load: 1 = the final windows were chosen from a warm-up proof's digit statistics (no re-tune follows) */
    int32_t warmup_proofs;    /* proofs finished in the warm-up arrangement */
    int32_t background_status; /* 0, or the cg_status the worker failed with (the context keeps proving in the warm-up arrangement) */
    int32_t reserved[3];
} cg_load_timings;
int cg_ctx_get_load_timings(cg_ctx* ctx, cg_load_timings* out);

/* Staged load: wait until the final arrangement is in force.  timeout_ms < 0 waits without limit.
 * Returns CG_OK when it is (at once for a synchronous load), 1 when the time ran out first, or the negative cg_status the
 * background part failed with (cg_last_error says why; the context keeps working in the warm-up arrangement). */
int cg_ctx_wait_ready(cg_ctx* ctx, int32_t timeout_ms);

/* Multi-GPU: a context loaded with shard_count > 1 owns a contiguous range of the l, a and b
 * queries and, of the h query, a contiguous range or — for a power-of-two shard_count — the coset points
 * j = shard_rank (mod shard_count), which lets two of its four transforms run at 1/shard_count of the size.  Which
 * points a shard owns is the library's business: the partial sums of all shards add up to the same five values.
 * cg_prove_partial computes this shard's five partial sums
 *   out = h ‖ l ‖ a ‖ b1 (4 x 64 B G1 affine canonical) ‖ b2 (128 B G2 affine canonical) = 384 B
 * (identity = zeros; b1 is all-zero and skipped when r == 0, prover.rs:102-112).
 * cg_assemble adds the gathered partials of all shards and finishes A, B, C exactly as
 * prover.rs:76-135.  partials: n_shards x 384 B. */
int cg_prove_partial(cg_ctx* ctx, const void* full_assignment, int assignment_on_device,
                     const uint8_t r[32], uint8_t out_partials[384], cg_timings* timings);
int cg_assemble(cg_ctx* ctx, const uint8_t* partials, uint32_t n_shards, const uint8_t r[32],
                const uint8_t s[32], uint8_t proof_out[256]);

/* SURVEY 8e's second arrangement of a sharded proof: the witness map runs ONCE (on one rank) and every shard receives the
 * scalars of its share of the h MSM, instead of every shard repeating the sparse products and the full-size transforms.
 * With the folded key (the default) those scalars are the coset values q_j = a(g w^j) b(g w^j) / Z(g), j < domain_size
 * (r1cs_to_qap.rs:187,201-208 without c's part, which the folded l query carries).
 *   cg_witness_map_coset : on a folded context WITHOUT CG_FLAG_H_SCALARS_EXTERNAL (whole or shard): all domain_size values,
 *       32 B canonical each, to host or device memory, laid out SHARD-MAJOR for this context's shard_count - shard p's
 *       scalars are the slice [offset_p, offset_p + count_p) that cg_h_scalars_slice reports (strided shards: q_{p + k·count},
 *       k < domain_size / count; contiguous shards and unsharded contexts: natural order) - so a scatter sends contiguous
 *       chunks.
 *   cg_prove_partial_q   : cg_prove_partial with this shard's slice supplied (host or device memory); the witness map is
 *       skipped.  Works on any shard context over a folded key; a context loaded with CG_FLAG_H_SCALARS_EXTERNAL can prove
 *       no other way.  The assignment is still checked for canonical elements (as the witness map would), the slice too. */
int cg_witness_map_coset(cg_ctx* ctx, const void* full_assignment, int assignment_on_device, void* q_out, int q_on_device);
int cg_h_scalars_slice(const cg_ctx* ctx, uint32_t shard, uint64_t* offset, uint64_t* count);
int cg_prove_partial_q(cg_ctx* ctx, const void* full_assignment, int assignment_on_device, const void* q_slice,
                       int q_on_device, const uint8_t r[32], uint8_t out_partials[384], cg_timings* timings);

/* The same in TWO CALLS, so that a shard's assignment-driven MSMs run WHILE the witness map and the scatter are still under way
 * somewhere else: of a sharded proof's critical path - witness map, scatter, partial sums - only the h share has to wait for
 * the slice (the l, a and b sums of prover.rs:74,266 need the assignment alone).
 *   cg_prove_partial_q_begin  : takes one of the context's proof slots, brings the assignment onto the GPU if it is not there,
 *       queues the l, a, b1 and b2 partial sums and RETURNS without waiting for them.  *out is the open proof.
 *   cg_partial_witness_map_coset : on the rank that runs the witness map (a context loaded WITHOUT CG_FLAG_H_SCALARS_EXTERNAL):
 *       cg_witness_map_coset for the open proof's assignment, on the open proof's own working set (a one-slot context has no other),
 *       next to the MSMs already queued.  Waits for the values.
 *   cg_prove_partial_q_finish : with this shard's slice (host or device memory): queues the h share, waits for everything, writes
 *       the 384-byte record, gives the slot back and destroys the handle - also when it fails.
 *   cg_prove_partial_q_abort  : for a caller that cannot deliver the slice: waits for what was queued, gives the slot back.
 * An open proof holds its slot: begin as many as the context has slots and no more, or begin blocks.  Calls on one handle are
 * the caller's to serialise; begin and finish may come from different threads.  Every open proof must be finished or aborted
 * before cg_circuit_free (which waits for the calls inside the context, open proofs included). */
/* The witness map in two HALVES (round 6).  Until their pointwise product the two sides of q_j = vinv·a(g w^j) · b(g w^j)
 * (r1cs_to_qap.rs:164-187) are independent - a sparse product with A (resp. B) and two transforms each - so two ranks can
 * compute one side each, at half the witness map's time, and every shard multiplies its two slices itself:
 *   cg_witness_map_coset_half / cg_partial_witness_map_coset_half : which = 0: the a side, vinv·a(g w^j); which = 1: the b side,
 *       b(g w^j); domain_size plain canonical values, laid out shard-major exactly as cg_witness_map_coset lays out q.
 *   cg_prove_partial_q_finish2 : cg_prove_partial_q_finish with the shard's slices of BOTH sides (both in host or both in device
 *       memory); the h scalars are their products mod r, formed on the GPU.  (The one-call form: begin, then finish2.) */
typedef struct cg_partial cg_partial;
int cg_witness_map_coset_half(cg_ctx* ctx, const void* full_assignment, int assignment_on_device, int which, void* out, int out_on_device);
int cg_partial_witness_map_coset_half(cg_partial* p, int which, void* out, int out_on_device);
int cg_prove_partial_q_finish2(cg_partial* p, const void* a_slice, const void* b_slice, int slices_on_device, uint8_t out_partials[384],
                               cg_timings* timings);
int cg_prove_partial_q_begin(cg_ctx* ctx, const void* full_assignment, int assignment_on_device, const uint8_t r[32], cg_partial** out);
int cg_partial_witness_map_coset(cg_partial* p, void* q_out, int q_on_device);
int cg_prove_partial_q_finish(cg_partial* p, const void* q_slice, int q_on_device, uint8_t out_partials[384], cg_timings* timings);
void cg_prove_partial_q_abort(cg_partial* p);

/* R1CS -> QAP witness map only: h coefficients, domain_size x 32 B canonical.
 * Replaces: `LibsnarkReduction::witness_map_from_matrices`, r1cs_to_qap.rs:150-213. */
int cg_witness_map(cg_ctx* ctx, const uint8_t* full_assignment, uint8_t* h_out);
uint64_t cg_domain_size(const cg_ctx* ctx);

/* The witness map over RESIDENT matrices, without a proving key: the reference's own plug point.
 * Replaces: an `impl R1CSToQAP` (forks/groth16/src/r1cs_to_qap.rs:49-98) whose `witness_map_from_matrices`
 *           (:150-213) is `Groth16<E, QAP>`'s type parameter (forks/groth16/src/lib.rs:55-57): a maintainer who only
 *           swaps the QAP type (INTEGRATION.md "GpuReduction") keeps arkworks' MSMs and moves the seven transforms
 *           and three sparse products here.  cg_qap_load copies the matrices once (the `cs.to_matrices()` product,
 *           r1cs_to_qap.rs:62); cg_qap_witness_map returns the reference's result, the coefficients of h
 *           (domain_size x 32 B canonical), for a full assignment in host or device memory.
 * Errors: CG_ERR_POLY_DEGREE_TOO_LARGE as r1cs_to_qap.rs:156-157; a non-canonical assignment element is
 *         CG_ERR_INVALID_ARGUMENT.  Calls on one handle serialise. */
typedef struct cg_qap_ctx cg_qap_ctx;
int cg_qap_load(cg_qap_ctx** out, const cg_csr abc[3], uint64_t num_inputs, uint64_t num_constraints,
                uint64_t num_variables, int32_t device /* -1 = current */);
int cg_qap_witness_map(cg_qap_ctx* ctx, const void* full_assignment, int assignment_on_device, void* h_out,
                       int h_on_device);
/* cg_check_witness on the key-less handle: where the reference's own check sits (the circom builder, before any key). */
int cg_qap_check_witness(cg_qap_ctx* ctx, const void* full_assignment, int assignment_on_device, cg_witness_report* report);
uint64_t cg_qap_domain_size(const cg_qap_ctx* ctx);
/* cg_qap_load with the form of the scalars that cross this handle: of the assignment cg_qap_witness_map and
 * cg_qap_check_witness take, and of the h_out cg_qap_witness_map writes (host or device memory alike; a device-resident
 * assignment is not written).  scalar_form = CG_FORM_MONTGOMERY is what an `impl R1CSToQAP` holds: `&[F]` in, `Vec<F>`
 * out, no `into_bigint` / `from_bigint` on either side.  cg_witness_report's a/b/c stay canonical.  A form above
 * CG_FORM_MONTGOMERY is CG_ERR_INVALID_ARGUMENT, reported before any HIP call.  cg_qap_load is this with CG_FORM_CANONICAL. */
int cg_qap_load_form(cg_qap_ctx** out, const cg_csr abc[3], uint64_t num_inputs, uint64_t num_constraints,
                     uint64_t num_variables, int32_t device /* -1 = current */, uint32_t scalar_form);
void cg_qap_free(cg_qap_ctx* ctx);

/* Unit level: Σ scalars[i]·bases[i] over BN254 G1 / G2 for caller-supplied bases.
 * Replaces: `<G as VariableBaseMSM>::msm_bigint(bases, scalars)` (ark-ec; call sites
 *           prover.rs:66,74,266).  bases in `coord_form`; scalars canonical; result affine
 *           canonical (64 / 128 B, zeros = identity).  Uses min(n_bases, n_scalars) pairs, as
 *           msm_bigint's zip does. */
int cg_msm_g1(const uint8_t* bases, uint32_t coord_form, uint64_t n_bases, const uint8_t* scalars,
              uint64_t n_scalars, int32_t window_bits, uint8_t out[64]);
int cg_msm_g2(const uint8_t* bases, uint32_t coord_form, uint64_t n_bases, const uint8_t* scalars,
              uint64_t n_scalars, int32_t window_bits, uint8_t out[128]);

/* n scalars from one form to the other (or copied, when the forms are equal), on the library's host threads.  Host only: no
 * HIP call, works in a process without a GPU.  in == out is allowed (other overlaps are not).  An input element >= r, in
 * either form, is CG_ERR_INVALID_ARGUMENT - cg_last_error names the index of the first one - and nothing is written.
 * For hosts that hold one form and need the other (a C host feeding a CG_FLAG_SCALARS_MONTGOMERY context, tests). */
int cg_scalars_convert(const uint8_t* in, uint32_t in_form, uint8_t* out, uint32_t out_form, uint64_t n);

/* Unit level: in-place radix-2 NTT over Fr, natural order in and out, 2^log_n x 32 B canonical.
 * Replaces: `EvaluationDomain::{fft,ifft}_in_place` and the coset variants obtained through
 *           `get_coset(F::GENERATOR)` (ark-poly; call sites r1cs_to_qap.rs:179-185,198-199,210).
 * inverse = 0: out[k] = Σ a[j] (g^j if coset) ω^{jk};  inverse = 1: the inverse map. */
int cg_ntt(uint8_t* data, uint32_t log_n, int inverse, int coset);

/* Unit level, resident operands: the handle forms of the two entry points above.  A caller that reuses a set
 * of bases (a query of the key, a commitment key) or a domain keeps the expanded window tables / twiddle tables
 * in HBM and may pass scalars / data that already live on the device; these run exactly the kernels cg_prove
 * runs and are what `tools/sweep.py` times (SURVEY 8d "unit sweeps").
 *   cg_msm_load_g1/g2 : opt may be NULL; opt->device and opt->window_bits are honoured (0 = size-based default), and of
 *                       opt->flags CG_FLAG_SCALARS_MONTGOMERY.
 *   cg_msm_run        : Σ scalars[i]·bases[i] over min(n_scalars, n_bases) pairs; scalars canonical (Montgomery on a
 *                       handle loaded with that flag: those pairs are converted, a device buffer is not written), host or
 *                       device memory; out = 64 B (G1) / 128 B (G2) affine canonical, zeros = identity.
 *                       timings (optional): the h (G1) or b2 (G2) MSM fields, accum_*, sort_ms, entries_*.
 *   cg_ntt_load/run   : in-place transform of 2^log_n canonical scalars in host or device memory, natural
 *                       order in and out; kernel_ms (optional) = HIP-event time of the transform's kernels.
 *                       A non-canonical element is CG_ERR_INVALID_ARGUMENT (device data is then unspecified).
 * Calls on one handle serialise; different handles are independent. */
typedef struct cg_msm_ctx cg_msm_ctx;
int cg_msm_load_g1(cg_msm_ctx** out, const uint8_t* bases, uint32_t coord_form, uint64_t n_bases, const cg_options* opt);
int cg_msm_load_g2(cg_msm_ctx** out, const uint8_t* bases, uint32_t coord_form, uint64_t n_bases, const cg_options* opt);
int cg_msm_run(cg_msm_ctx* ctx, const void* scalars, int scalars_on_device, uint64_t n_scalars, uint8_t* out,
               cg_timings* timings);
void cg_msm_free(cg_msm_ctx* ctx);
typedef struct cg_ntt_ctx cg_ntt_ctx;
int cg_ntt_load(cg_ntt_ctx** out, uint32_t log_n, int32_t device /* -1 = current */);
int cg_ntt_run(cg_ntt_ctx* ctx, void* data, int data_on_device, int inverse, int coset, float* kernel_ms);
void cg_ntt_free(cg_ntt_ctx* ctx);

/* out[i] = scalars[i]·G for the standard generator of G1 / G2 (canonical scalars in, canonical affine points
 * out, 64 / 128 B each, zeros = identity).
 * Replaces: `FixedBase::msm::<E::G1 | E::G2>(scalar_bits, window, &table, &scalars)` [ark-ec], the building block
 *           of the generator (forks/groth16/src/generator.rs:134-140,147-148,162-194). */
int cg_fixed_base_g1(const uint8_t* scalars, uint64_t n, uint8_t* out);
int cg_fixed_base_g2(const uint8_t* scalars, uint64_t n, uint8_t* out);

/* Trusted setup from explicit toxic waste, on the GPU.
 * Replaces: `generate_parameters_with_qap`, forks/groth16/src/generator.rs:50-228, with
 *           gamma = 1 and the standard generators as the fork fixes them (:28,:34-35).
 * Outputs are written canonical into caller buffers sized as in cg_proving_key;
 * gamma_abc_g1 gets num_inputs x 64 B (vk.gamma_abc_g1), vk_points gets
 * alpha_g1(64) ‖ beta_g1(64) ‖ delta_g1(64) ‖ beta_g2(128) ‖ gamma_g2(128) ‖ delta_g2(128). */
int cg_setup(const cg_csr abc[3], uint64_t num_inputs, uint64_t num_constraints,
             uint64_t num_variables, const uint8_t tau[32], const uint8_t alpha[32],
             const uint8_t beta[32], const uint8_t delta[32], uint8_t* a_query, uint8_t* b_g1_query,
             uint8_t* b_g2_query, uint8_t* h_query, uint8_t* l_query, uint8_t* gamma_abc_g1,
             uint8_t vk_points[576]);

/* .r1cs (iden3 binary) -> CSR.  Replaces: `R1CSFile::new` + `R1CS::from`,
 * forks/circom-compat/src/circom/r1cs_reader.rs:54-148,26-38.
 * The returned object owns its arrays; cg_r1cs_csr fills views valid until cg_r1cs_free. */
typedef struct cg_r1cs cg_r1cs;
typedef struct cg_r1cs_header {
    uint32_t field_size, n_wires, n_pub_out, n_pub_in, n_prv_in, n_constraints;
    uint64_t n_labels;
    uint64_t num_inputs;      /* 1 + n_pub_in + n_pub_out  (r1cs_reader.rs:28) */
    uint64_t num_variables;   /* n_wires */
} cg_r1cs_header;
int cg_r1cs_parse(const uint8_t* data, uint64_t len, cg_r1cs** out);
int cg_r1cs_get(const cg_r1cs* r, cg_r1cs_header* header, cg_csr abc[3], const uint64_t** wire_mapping);
void cg_r1cs_free(cg_r1cs* r);

/* ark-serialize (uncompressed) proving key <-> packed arrays.
 * Replaces: `read_from_file::<ProverParams>` / `write_to_file` for the `groth16_params: ProvingKey<Bn254>` that
 *           leads creds' prover_params.bin (creds/src/utils.rs:140-152,179-189; creds/src/lib.rs:58-63;
 *           field order forks/groth16/src/data_structures.rs:31-44,101-118).  Parsing is the reference's
 *           `deserialize_uncompressed_unchecked`: flags stripped, no curve / subgroup checks.
 * cg_pk_parse reads one ProvingKey from the start of `data` (bytes_consumed, optional, tells where the
 * PreparedVerifyingKey / config string that follow in prover_params.bin begin); cg_pk_get fills a view valid
 * until cg_pk_free, plus the verifying-key members the prover itself does not need. */
typedef struct cg_pk cg_pk;
int cg_pk_parse(const uint8_t* data, uint64_t len, cg_pk** out, uint64_t* bytes_consumed);
int cg_pk_get(const cg_pk* k, cg_proving_key* view, const uint8_t** gamma_g2, const uint8_t** gamma_abc_g1,
              uint64_t* gamma_abc_len);
void cg_pk_free(cg_pk* k);
uint64_t cg_pk_serialized_size(const cg_proving_key* pk, uint64_t gamma_abc_len);
int cg_pk_serialize(const cg_proving_key* pk, const uint8_t* gamma_g2, const uint8_t* gamma_abc_g1,
                    uint64_t gamma_abc_len, uint8_t* out, uint64_t out_len);

/* prover_params.bin: `ProverParams { groth16_params: ProvingKey, groth16_pvk: PreparedVerifyingKey,
 * config_str: String }`.
 * Replaces: `read_from_file::<ProverParams>` in `create_client_state` (creds/src/lib.rs:58-63,268;
 *           creds/src/utils.rs:179-189) and `write_to_file(&prover_params, ..)` in `run_zksetup` (creds/src/lib.rs:245-248).
 * The prover consumes the key; the serialized VerifyingKey, PreparedVerifyingKey (data_structures.rs:62-71: vk, an Fq12
 * and two bn::G2Prepared) and the configuration string are returned verbatim, because `create_client_state` copies
 * them into the ClientState (creds/src/lib.rs:292-299).  Views stay valid until cg_prover_params_free. */
typedef struct cg_prover_params cg_prover_params;
typedef struct cg_prover_params_view {
    cg_proving_key pk;               /* canonical packed arrays, as cg_pk_get */
    const uint8_t* gamma_g2;         /* vk.gamma_g2, 128 B */
    const uint8_t* gamma_abc_g1;     /* vk.gamma_abc_g1, gamma_abc_len x 64 B */
    uint64_t gamma_abc_len;
    const uint8_t* vk_bytes;  uint64_t vk_len;      /* groth16_params.vk as serialized */
    const uint8_t* pvk_bytes; uint64_t pvk_len;     /* groth16_pvk as serialized */
    const uint8_t* config_str; uint64_t config_len; /* UTF-8, no terminator */
} cg_prover_params_view;
int cg_prover_params_parse(const uint8_t* data, uint64_t len, cg_prover_params** out);
int cg_prover_params_get(const cg_prover_params* pp, cg_prover_params_view* view);
void cg_prover_params_free(cg_prover_params* pp);
uint64_t cg_prover_params_serialized_size(const cg_proving_key* pk, uint64_t gamma_abc_len, uint64_t pvk_len,
                                          uint64_t config_len);
int cg_prover_params_serialize(const cg_proving_key* pk, const uint8_t* gamma_g2, const uint8_t* gamma_abc_g1,
                               uint64_t gamma_abc_len, const uint8_t* pvk_bytes, uint64_t pvk_len,
                               const uint8_t* config_str, uint64_t config_len, uint8_t* out, uint64_t out_len);

/* client_state.bin: the hand-over from the prove step to the host-side `show` step.
 * Replaces: `ClientState::<E>::new` + `write_to_file` / `new_from_file` (creds/src/groth16rand.rs:23-35,60-98;
 *           creds/src/lib.rs:292-300), ark-serialize uncompressed, fields in declaration order:
 *           inputs: Vec<Fr> | aux: Option<String> | proof | vk | pvk | input_com_randomness: Option<Fr> |
 *           committed_input_openings: Vec<PedersenOpening<G1>> (creds/src/dlog.rs:24-29) | credtype | config_str.
 * The library writes the 256-byte proof cg_prove returned next to the vk / pvk / config bytes that came out of
 * prover_params.bin; openings (empty for a fresh state) travel as their serialized bytes. */
typedef struct cg_client_state cg_client_state;
typedef struct cg_client_state_view {
    const uint8_t* inputs; uint64_t n_inputs;        /* public inputs (wires 1 .. num_inputs-1), 32 B canonical each */
    const uint8_t* aux; uint64_t aux_len; int32_t has_aux;
    int32_t has_input_com_randomness;
    const uint8_t* proof;                            /* 256 B */
    const uint8_t* vk_bytes; uint64_t vk_len;
    const uint8_t* pvk_bytes; uint64_t pvk_len;
    const uint8_t* input_com_randomness;             /* 32 B when has_input_com_randomness */
    const uint8_t* openings_bytes; uint64_t openings_len; uint64_t n_openings;
    const uint8_t* credtype; uint64_t credtype_len;  /* "jwt" (groth16rand.rs:76) or "mdl" */
    const uint8_t* config_str; uint64_t config_len;
} cg_client_state_view;
uint64_t cg_client_state_serialized_size(const cg_client_state_view* v);
int cg_client_state_serialize(const cg_client_state_view* v, uint8_t* out, uint64_t out_len);
int cg_client_state_parse(const uint8_t* data, uint64_t len, cg_client_state** out);
int cg_client_state_get(const cg_client_state* cs, cg_client_state_view* view);
void cg_client_state_free(cg_client_state* cs);

/* Groth16 verification (SURVEY 8f-2's last step: what create_client_state runs after the prove, creds/src/lib.rs:286-290).
 * Verdicts: one byte per proof.  CG_VERIFY_MALFORMED = the proof or its public inputs fail ark's CHECKED
 * deserialisation (a coordinate >= q, a bad flag combination, A or C off the curve, B off the twist or outside the
 * r-torsion, an input >= r) - for that proof only; a proof from cg_prove always passes these checks. */
enum { CG_VERIFY_REJECT = 0, CG_VERIFY_ACCEPT = 1, CG_VERIFY_MALFORMED = 2 };
typedef struct cg_pvk cg_pvk;
/* Replaces: `PreparedVerifyingKey::deserialize_uncompressed_unchecked` (creds/src/utils.rs:186) + the upload to a device
 *           (device -1 = current).  Bytes that are not exactly one PreparedVerifyingKey (data_structures.rs:62-71) are
 *           CG_ERR_PARSE, reported before any HIP call; an empty gamma_abc_g1 is CG_ERR_MALFORMED_KEY. */
int cg_pvk_load(cg_pvk** out, const uint8_t* pvk_bytes, uint64_t len, int32_t device);
/* gamma_abc_g1.len() - 1: the public inputs a proof under this key carries */
int cg_pvk_num_inputs(const cg_pvk* k, uint64_t* n);
/* How a key handle arranges the pairing stage (Miller loop, final exponentiation) of its verifying calls.
 * 0 (default) = one lane per proof: any batch up to the chunk (32768) costs what one proof costs, which suits batches.
 * 1 = one workgroup per proof (csrc/pairing_team.hpp): a lone proof is answered sooner, large batches more slowly; on a
 *     cg_pvk the [r]B = O chain then also runs beside the pairing on a second stream of the handle instead of before it.
 * Measured on an MI355X (profiles/verify_lone.md): a lone Groth16 proof with 26 inputs takes 21 ms instead of 72 ms, a
 * lone 32-bit range proof 24 ms instead of 50 ms; the latency arrangement stays ahead up to n = 1024 (33 against 65 ms,
 * 32 against 45 ms) and the wide one overtakes it between n = 1024 and n = 4096, at about 3000 proofs.  Switch a handle
 * on when it answers one request at a time.  The mode is a property of the handle, taken under its lock; with it on, every call on
 * the handle uses it whatever its n.  Verdict and k_out bytes are identical in both modes for every input.  A value other
 * than 0 or 1, or a null handle, is CG_ERR_INVALID_ARGUMENT.  (No counterpart in the reference.) */
int cg_pvk_set_latency_mode(cg_pvk* k, int32_t on);
/* as cg_range_vk_last_kernel_ms, for cg_verify_batch / cg_verify_show_batch: (group stage, pairing) of the last call */
int cg_pvk_last_kernel_ms(cg_pvk* k, float* group_ms, float* pairing_ms);
/* Replaces: `Groth16::verify_with_processed_vk` for n proofs under one key (forks/groth16/src/verifier.rs:25-65).
 * inputs: n x n_inputs x 32 B canonical Fr; proofs: n x 256 B (cg_prove's layout, ark-serialize uncompressed a ‖ b ‖ c);
 * verdicts: n bytes, CG_VERIFY_*.  n_inputs + 1 != gamma_abc_g1.len() is CG_ERR_MALFORMED_KEY
 * (SynthesisError::MalformedVerifyingKey).  Any n; calls on one handle serialise, different handles are independent. */
int cg_verify_batch(cg_pvk* k, const uint8_t* inputs, uint64_t n_inputs, const uint8_t* proofs, uint64_t n,
                    uint8_t* verdicts);
/* Replaces: `ShowGroth16::verify` (creds/src/groth16rand.rs:232-306, called at creds/src/lib.rs:630 and :832) for n
 * showings under one key and ONE io_types layout (an endpoint has one proof spec), up to the Merlin transcript:
 *   - the Groth16 half entirely: the prepared inputs com_hidden + gamma_abc[0] + sum committed_i +
 *     sum_{revealed j} x_j * gamma_abc[j+1] (:246-279), then `verify_proof_with_prepared_inputs`
 *     (forks/groth16/src/verifier.rs:44-65) -> verdicts[i];
 *   - the group arithmetic of `DLogPoK::verify` (creds/src/dlog.rs:134-153): per statement i the recomputed Schnorr
 *     commitment k_i = sum_j s_ij * base_ij + c * y_i, written to k_out as the 32 bytes `add_to_transcript(b"k", ..)`
 *     appends (ark-serialize COMPRESSED G1).  y_i is the i-th committed point, com_hidden for the last statement.
 * NOT done here: the transcript itself and the comparison `c == self.c` (dlog.rs:130-132,147-152,166-174).  The host
 * feeds the bases, k_out and y into its own Merlin transcript and compares the challenge; a showing is valid when its
 * verdict is CG_VERIFY_ACCEPT and that comparison holds ("Verifying showings").
 * io_types: one byte per public input (creds/src/structs.rs:33-37), n_io must equal cg_pvk_num_inputs, else
 *   CG_ERR_MALFORMED_KEY; a byte above 2 is CG_ERR_INVALID_ARGUMENT.  With n_revealed / n_hidden / n_committed of each:
 * revealed:    n x n_revealed x 32 B canonical Fr, in input order (:260-264)
 * rand_proofs: n x 256 B, cg_prove's layout
 * com_hidden:  n x 64 B ark-serialize uncompressed G1;  committed: n x n_committed x 64 B, same, in input order
 * pok_c:       n x 32 B canonical Fr; NULL = the Groth16 half only (pok_s and k_out are then not touched)
 * pok_s:       n x n_resp x 32 B, n_resp = 2 * n_committed + n_hidden + 1, statement-major as dlog.rs:135-145 reads them:
 *              per committed input the response for gamma_abc[i+1], then for delta_g1 (:272-275); then one per hidden
 *              input, then the one for delta_g1 (:266,280)
 * verdicts:    n x CG_VERIFY_*;  k_out: n x (n_committed + 1) x 32 B
 * CG_VERIFY_MALFORMED (that showing only, its k_out bytes zero): rand_proof fails cg_verify_batch's checks, com_hidden
 * or a committed point fails ark's checked G1 deserialisation, or a revealed input, a response or c is >= r.
 * Argument errors are reported before any HIP call; n = 0 is CG_OK. */
enum { CG_IO_REVEALED = 0, CG_IO_HIDDEN = 1, CG_IO_COMMITTED = 2 };
int cg_verify_show_batch(cg_pvk* k, const uint8_t* io_types, uint64_t n_io, const uint8_t* revealed,
                         const uint8_t* rand_proofs, const uint8_t* com_hidden, const uint8_t* committed,
                         const uint8_t* pok_c, const uint8_t* pok_s, uint64_t n, uint8_t* verdicts, uint8_t* k_out);
/* Creating showings: `ClientState::show_groth16` (creds/src/groth16rand.rs:100-187) for n client states under one key and
 * ONE io_types layout, in two calls around the host's Merlin transcript.  The library draws no randomness and runs no
 * transcript: every random scalar comes from the caller (as r, s of cg_prove do), and between the two calls the host
 * absorbs the bases, k_out and the committed points / com_hidden into its own Merlin transcript and squeezes c
 * (creds/src/dlog.rs:56-99; INTEGRATION.md, "Creating showings").
 * A showing consumes n_rand = 3 + n_committed + n_resp scalars (n_resp = 2 * n_committed + n_hidden + 1), in this order:
 *   r1, r2 (rerandomize_proof) | r_i per committed input, in input order | z (input_com_randomness) |
 *   the n_resp nonces, statement-major as dlog.rs:60-67 draws them: per committed input (for gamma_abc[i+1], for
 *   delta_g1), then one per hidden input, then one for delta_g1. */
enum { CG_SHOW_MADE = 1, CG_SHOW_MALFORMED = 2 };
/* A third status byte, of cg_p256_rtu_batch alone: the row is well formed and its ECDSA signature does not verify. */
enum { CG_P256_BAD_SIGNATURE = 3 };
/* The n_rand of a layout.  Host only. */
int cg_show_rand_count(const uint8_t* io_types, uint64_t n_io, uint64_t* n_rand);
/* Replaces: `rerandomize_proof` (forks/groth16/src/prover.rs:227-254), the Pedersen commitments and com_hidden_inputs of
 * groth16rand.rs:120-160, the correction of C (:167-168) and the commitments k_i of `DLogPoK::prove` (dlog.rs:60-75), on
 * the GPU.
 * proofs: n x 256 B (cg_prove's layout);  inputs: n x n_io x 32 B canonical Fr (`ClientState.inputs`; only hidden and
 * committed positions are read);  rand: n x n_rand x 32 B canonical Fr, as above.
 * rand_proofs: n x 256 B, A' = r1^-1 A | B' = r1 (B + r2 delta_g2) | C'' = C + r2 A - (sum r_i + z) G
 * com_hidden:  n x 64 B, sum x_j gamma_abc[j+1] + z delta_g1 over the hidden inputs
 * committed:   n x n_committed x 64 B, x_i gamma_abc[i+1] + r_i delta_g1
 *   (all ark-serialize uncompressed, the bytes cg_verify_show_batch takes back)
 * k_out:       n x (n_committed + 1) x 32 B, k_i = sum_j rho_ij base_ij as ark-serialize COMPRESSED G1: what
 *              `add_to_transcript(b"k", ..)` appends, the encoding cg_verify_show_batch's k_out has
 * status:      n x CG_SHOW_*.  CG_SHOW_MALFORMED (that showing only, all of its outputs zero bytes): a proof coordinate
 *              >= q, bad point flags, A or C off the curve, B off the twist (B's subgroup is NOT checked: a client state is
 *              the host's own data, which the reference reads unchecked); a read input or a rand scalar >= r; r1 = 0 or
 *              r2 = 0 (the reference redraws those, prover.rs:234-237).
 * n_io != cg_pvk_num_inputs is CG_ERR_MALFORMED_KEY, a byte above 2 in io_types CG_ERR_INVALID_ARGUMENT; a key whose
 * gamma_g2 is not the G2 generator is CG_ERR_MALFORMED_KEY (the correction of C holds for the fork's gamma = 1 keys only,
 * forks/groth16/src/generator.rs:28).  Argument errors are reported before any HIP call; n = 0 is CG_OK. */
int cg_show_commit_batch(cg_pvk* k, const uint8_t* io_types, uint64_t n_io, const uint8_t* proofs,
                         const uint8_t* inputs, const uint8_t* rand, uint64_t n, uint8_t* rand_proofs,
                         uint8_t* com_hidden, uint8_t* committed, uint8_t* k_out, uint8_t* status);
/* Replaces: the responses of `DLogPoK::prove` (dlog.rs:101-109), s_ij = rho_ij - c * secret_ij mod r, once the host's
 * Merlin transcript has produced c.  Host only, on the calling thread: no handle, no HIP call.
 * inputs, rand: as given to cg_show_commit_batch;  pok_c: n x 32 B canonical Fr;  status: that call's status bytes, or
 * NULL for "all made" - a showing whose byte is not CG_SHOW_MADE is not read and gets zero bytes.
 * pok_s: n x n_resp x 32 B in the order cg_verify_show_batch reads them (secrets: x_i, r_i per committed input, then the
 * hidden x_j, then z).  A value >= r in a showing that is read, its c included, is CG_ERR_INVALID_ARGUMENT naming the
 * showing, and nothing is written. */
int cg_show_respond_batch(const uint8_t* io_types, uint64_t n_io, const uint8_t* inputs, const uint8_t* rand,
                          const uint8_t* pok_c, const uint8_t* status, uint64_t n, uint8_t* pok_s);
void cg_pvk_free(cg_pvk* k);

/* Creating range proofs: `ClientState::show_range` (creds/src/groth16rand.rs:193-229) -> `RangeProof::prove_n_bits`
 * (creds/src/rangeproof.rs:114-339) for n Pedersen openings under one KZG key, the other half of a showing
 * (creds/src/lib.rs:373, :471, :509), in three GPU calls around the host's Merlin transcripts and one host-only call.  As
 * with showings the library draws no randomness and runs no transcript:
 *
 *               com_f, com_g, k_0, k_1 --> DLEQ transcript  --> c_dleq      (dlog.rs:56-99)
 *   commit  --> com_f, com_g ------------> range transcript --> c           (rangeproof.rs:250-257)
 *   quotient (c) --> com_q --------------> range transcript --> rho         (:270-274)
 *   open (c, rho) --> eval_g, proof_g, eval_gw, proof_gw, eval_w_hat, proof_w_hat   (:277-325)
 *   respond (c_dleq) --> s = nonce - c_dleq * secret                        (dlog.rs:101-109)
 *
 * The three GPU calls are stateless: each recomputes what it needs from openings, rand and the challenges, as
 * cg_show_respond_batch re-reads its inputs; nothing is kept on the handle between calls ("Creating range
 * proofs").
 * openings: n x 2 x 32 B canonical Fr, `ped_open.m` and `ped_open.r` (dlog.rs:24-29).
 * rand:     n x CG_RANGE_N_RAND x 32 B canonical Fr, in the order the reference draws them:
 *   b0 b1 b2 (the blinding of g, rangeproof.rs:169-170) | f0 f1 f2 (rand_f, :216) | t_m t_r (the nonces of the DLEQ's
 *   statement 0, dlog.rs:60-67) | t_f0 t_f1 t_f2 (of statement 1; its fourth nonce is t_m, eq_pos = (0, 3), and is not
 *   supplied) | g0 g1 g2 g3 (rand_g, rangeproof.rs:248) | q0 q1 q2 (rand_q, :268)
 * status:   n x CG_SHOW_MADE / CG_SHOW_MALFORMED, written by each call from its own inputs.  A malformed showing gets
 *   zero bytes in every output of that call and leaves its neighbours alone.  Malformed: any scalar the call reads >= r;
 *   m >= 2^n_bits (the reference asserts against it, groth16rand.rs:202-204); f0..f2 all zero, g0..g3 all zero or q0..q2
 *   all zero (the reference would emit a non-hiding commitment and `random_v = None`); in cg_range_open_batch rho^n_bits
 *   = 1, which covers rho = 1, where the reference divides by zero (rangeproof.rs:293).
 * DEVIATION: `random_v` is always written.  The reference writes `None` for proof_w_hat only when f_coeff * rand_f +
 *   q_coeff * rand_q cancels to the zero polynomial (kzg10/mod.rs:287-291); that showing is made here with random_v = 0 and
 *   a W without hiding term, which is the same group element and evaluation.
 * Argument errors (a null array, an unknown slot) are reported before any HIP call; n = 0 is CG_OK; calls on one handle
 * serialise, different handles are independent. */
typedef struct cg_range_pk cg_range_pk;
enum { CG_RANGE_N_RAND = 18, CG_RANGE_N_RESP = 6 };
/* Replaces: `read_from_file` of range_pk.bin (creds/src/lib.rs:241; `Powers`, forks/ark-poly-commit/src/kzg10/
 *           data_structures.rs:144-176: u64 length and that many 64-byte ark-uncompressed G1 points for powers_of_g, then
 *           the same for powers_of_gamma_g), read unchecked as the reference does, + the upload to a device (-1 = current)
 *           of fixed-base tables of powers_of_g[0..2 n_bits + 3] and powers_of_gamma_g[0..3]: deg q = deg w_hat =
 *           2 n_bits + 3, so these are all the powers prove_n_bits reaches (36 MB at n_bits = 32).
 * Bytes that are not exactly that are CG_ERR_PARSE; n_bits outside {2, 4, 8, 16, 32} is CG_ERR_INVALID_ARGUMENT (the
 * reference takes a power of two, RANGE_PROOF_INTERVAL_BITS = 32); fewer than 2 n_bits + 4 powers of g or 4 of gamma_g is
 * CG_ERR_MALFORMED_KEY.  All of them are reported before any HIP call. */
int cg_range_pk_load(cg_range_pk** out, const uint8_t* range_pk_bytes, uint64_t len, uint32_t n_bits, int32_t device);
/* Registers one pair of Pedersen bases - an input's `gamma_abc_g1[pos]` and `delta_g1` (groth16rand.rs:135-139, :319-323), 2 x 64 B
 * ark-serialize uncompressed - builds their tables and returns the slot cg_range_commit_batch takes.  An mdl endpoint
 * registers one pair per range-checked attribute; up to 64 slots.  A point that fails ark's checked G1 deserialisation
 * is CG_ERR_INVALID_ARGUMENT. */
int cg_range_pk_add_bases(cg_range_pk* k, const uint8_t ped_bases[128], uint32_t* slot);
void cg_range_pk_free(cg_range_pk* k);
/* Diagnostic: the HIP-event time of the two kernels (the polynomial stage, the fixed-base walks) of the handle's last GPU
 * call, summed over its chunks.  (No counterpart in the reference.) */
int cg_range_pk_last_kernel_ms(cg_range_pk* k, float* poly_ms, float* points_ms);
/* Replaces: the commitments of prove_n_bits before its first challenge: `KZG10::commit` of f = m and of g blinded
 *           (rangeproof.rs:143-172, :216, :248; kzg10/mod.rs:178-241) and the commitments k_0, k_1 of the DLEQ's
 *           `DLogPoK::prove` (rangeproof.rs:218-245, dlog.rs:60-91), on the GPU.
 * com_f, com_g: n x 64 B ark-serialize uncompressed.
 * ts_out: n x 4 x 32 B ark-serialize COMPRESSED G1, the bytes `add_to_transcript` appends (utils.rs:29-37): com_f, com_g
 *         (both transcripts' view of them), k_0 = t_m B_0 + t_r B_1 over the slot's bases, k_1 = t_f0 gamma_g[0] +
 *         t_f1 gamma_g[1] + t_f2 gamma_g[2] + t_m g[0]. */
int cg_range_commit_batch(cg_range_pk* k, uint32_t slot, const uint8_t* openings, const uint8_t* rand, uint64_t n,
                          uint8_t* com_f, uint8_t* com_g, uint8_t* ts_out, uint8_t* status);
/* Replaces: q1, q2, q3, q = q1 + c q2 + c^2 q3 and `KZG10::commit` of q (rangeproof.rs:183-213, :258-268).
 * c: n x 32 B canonical Fr.  com_q: n x 64 B uncompressed;  ts_q: n x 32 B, com_q compressed. */
int cg_range_quotient_batch(cg_range_pk* k, const uint8_t* openings, const uint8_t* rand, const uint8_t* c, uint64_t n,
                            uint8_t* com_q, uint8_t* ts_q, uint8_t* status);
/* Replaces: the three evaluations and `KZG10::open` calls of rangeproof.rs:277-325 (kzg10/mod.rs:247-331).
 * c, rho: n x 32 B canonical Fr.  evals: n x 3 x 32 B: eval_g, eval_gw, eval_w_hat.  proofs: n x 3 x 96 B, each
 * W (64 B uncompressed) ‖ random_v (32 B), for proof_g, proof_gw, proof_w_hat. */
int cg_range_open_batch(cg_range_pk* k, const uint8_t* openings, const uint8_t* rand, const uint8_t* c, const uint8_t* rho,
                        uint64_t n, uint8_t* evals, uint8_t* proofs, uint8_t* status);
/* Replaces: the responses of the DLEQ's `DLogPoK::prove` (dlog.rs:101-109) once the host's transcript has produced
 *           c_dleq.  Host only, on the calling thread, as cg_show_respond_batch: no handle, no HIP call.
 * status: cg_range_commit_batch's bytes, or NULL for "all made"; a showing whose byte is not CG_SHOW_MADE is not read and
 * gets zero bytes.  pok_s: n x CG_RANGE_N_RESP x 32 B: s_00, s_01 (secrets m, r), then s_10..s_13 (f0, f1, f2, m); s_13
 * equals s_00.  A value >= r in a showing that is read, its c_dleq included, is CG_ERR_INVALID_ARGUMENT naming the
 * showing, and nothing is written. */
int cg_range_respond_batch(const uint8_t* openings, const uint8_t* rand, const uint8_t* c_dleq, const uint8_t* status,
                           uint64_t n, uint8_t* pok_s);

/* Verifying range proofs: `ShowRange::verify` (creds/src/lib.rs:650, :852, :881) -> `RangeProof::verify_n_bits`
 * (creds/src/rangeproof.rs:342-424) for n proofs under one `RangeProofVK`, the other half of verifying a showing beside
 * cg_verify_show_batch.  The split is the same: the group arithmetic, the pairing check of `KZG10::batch_check`
 * (forks/ark-poly-commit/src/kzg10/mod.rs:357-411), the evaluation identity (rangeproof.rs:395-412) and the DLEQ's eq_pos
 * comparison (dlog.rs:155-164) run on the GPU; every Merlin transcript and the final `c == self.c` stay with the host
 * ("Verifying range proofs"):
 *
 *   com_f, com_g (compressed) --> range transcript --> c;  com_q --> rho      (rangeproof.rs:352-366)
 *   verify (c, rho, r_1, r_2) --> verdicts, k_0, k_1
 *   bases, k_i, y_i ------------> DLEQ transcript --> c' == pok_c ?           (dlog.rs:130-174)
 *
 * The library draws no randomness: batch_check's randomizers r_1, r_2 (`u128::rand`, kzg10/mod.rs:390; r_0 = 1) are the
 * caller's, as r, s of cg_prove are.  They must be unpredictable to whoever made the proofs. */
typedef struct cg_range_vk cg_range_vk;
/* Replaces: `read_from_file` of range_vk.bin (`RangeProofVK`, rangeproof.rs:74-78): the KZG `VerifierKey` as its
 *           hand-written serialisation writes it (kzg10/data_structures.rs:217-264: g 64 B | gamma_g 64 B | h 128 B |
 *           beta_h 128 B, ark-serialize uncompressed) and com_f_basis as four uncompressed G1 points with no length
 *           prefix: 640 bytes exactly, read unchecked as the reference reads them; prepared_h and prepared_beta_h are
 *           computed here as the reference's deserialiser computes them (a G2 point at infinity gives a prepared point
 *           marked infinity, whose pair the pairing check skips) + the upload to a device (-1 = current) of both and of
 *           fixed-base tables of g, gamma_g and com_f_basis.
 * Another length, a coordinate >= q or invalid point flags are CG_ERR_PARSE; n_bits outside {2, 4, 8, 16, 32} is
 * CG_ERR_INVALID_ARGUMENT.  All of them are reported before any HIP call. */
int cg_range_vk_load(cg_range_vk** out, const uint8_t* range_vk_bytes, uint64_t len, uint32_t n_bits, int32_t device);
/* As cg_range_pk_add_bases: registers an input's `gamma_abc_g1[pos]` and `delta_g1` (groth16rand.rs:319-323), the bases of
 * the Pedersen commitment a range proof speaks about, 2 x 64 B ark-serialize uncompressed, checked; up to 64 slots. */
int cg_range_vk_add_bases(cg_range_vk* k, const uint8_t ped_bases[128], uint32_t* slot);
/* Diagnostic: the HIP-event time of the handle's last call, summed over its chunks: the group stage (checks, scalar
 * multiplications, sums) and the pairing (Miller loop, final exponentiation).  (No counterpart in the reference.) */
int cg_range_vk_last_kernel_ms(cg_range_vk* k, float* group_ms, float* pairing_ms);
/* as cg_pvk_set_latency_mode, for cg_range_verify_batch: the pairing of each showing on one workgroup; the group stage
 * stays as it is */
int cg_range_vk_set_latency_mode(cg_range_vk* k, int32_t on);
void cg_range_vk_free(cg_range_vk* k);
/* Replaces: `verify_n_bits` between its transcripts, for n proofs whose commitment has the bases of `slot`.  The pieces
 *           of a `RangeProof` come in the layouts the cg_range_* creation calls write, so a round trip repacks nothing:
 * ped_com, com_f, com_g, com_q: n x 64 B ark-serialize uncompressed G1 (ped_com: the Pedersen commitment, y_0 of the DLEQ)
 * evals:       n x 3 x 32 B canonical Fr: eval_g, eval_gw, eval_w_hat
 * proofs:      n x 3 x 96 B: W (64 B uncompressed) ‖ random_v (32 B) of proof_g, proof_gw, proof_w_hat; a random_v of
 *              `None` is passed as 0, which is the same group element
 * c, rho:      n x 32 B canonical Fr, the range transcript's two challenges
 * randomizers: n x 2 x 16 B little-endian u128: r_1, r_2; any value, 0 included
 * pok_c:       n x 32 B, the DLEQ's c (dleq_proof.c); NULL = steps up to the evaluation identity only: ped_com, pok_s and
 *              k_out are then not touched
 * pok_s:       n x CG_RANGE_N_RESP x 32 B: s_00 s_01 s_10..s_13, as cg_range_respond_batch writes them
 * verdicts:    n x CG_VERIFY_*.  CG_VERIFY_ACCEPT: e(-total_w, beta_h) e(total_c, h) = 1, the evaluation identity holds and
 *              (with a DLEQ) s_00 == s_13; the showing is valid when the host's recomputed DLEQ challenge also equals
 *              pok_c.  CG_VERIFY_REJECT: one of the three fails.  CG_VERIFY_MALFORMED (that showing only, its k_out bytes
 *              zero, its neighbours untouched): one of the seven points fails ark's checked G1 deserialisation (a
 *              coordinate >= q, invalid flags, off the curve; the identity is legal), a scalar is >= r, or rho is 1 or
 *              w^(n_bits - 1), the two values at which the reference divides by zero and panics.  Every other rho with
 *              rho^n_bits = 1 is computed as the reference computes it (q_coeff = f_coeff = 0, com_w_hat = O).
 * k_out:       n x 2 x 32 B ark-serialize COMPRESSED G1: k_0 = s_00 B_0 + s_01 B_1 + c ped_com and k_1 = s_10 gamma_g[0] +
 *              s_11 gamma_g[1] + s_12 gamma_g[2] + s_13 g[0] + c com_f (dlog.rs:135-145), the bytes
 *              `add_to_transcript(b"k", ..)` appends, in the encoding of cg_range_commit_batch's ts_out[2..3].
 * Argument errors (a null array, an unknown slot) are reported before any HIP call; n = 0 is CG_OK; calls on one handle
 * serialise, different handles are independent. */
int cg_range_verify_batch(cg_range_vk* k, uint32_t slot, const uint8_t* ped_com, const uint8_t* com_f, const uint8_t* com_g,
                          const uint8_t* com_q, const uint8_t* evals, const uint8_t* proofs, const uint8_t* c, const uint8_t* rho,
                          const uint8_t* randomizers, const uint8_t* pok_c, const uint8_t* pok_s, uint64_t n, uint8_t* verdicts,
                          uint8_t* k_out);

/* Range proofs in one call each way, with the library's own Merlin.  The transcripts of `prove_n_bits` and
 * `verify_n_bits` - STROBE-128 over Keccak-f[1600] as the `merlin` crate computes them, every message the value's
 * ark-serialize compressed bytes (creds/src/utils.rs:29-37), every challenge 31 bytes read little-endian - run on the
 * device between the kernels of the calls above, so a proof is made, or checked, without a host step in between
 * ("Range proofs in one call").  The multi-call entries above stay for hosts that run their own
 * transcripts.
 *
 * Replaces: `RangeProof::prove_n_bits` (rangeproof.rs:114-339) whole, for n openings whose commitment has the bases of
 *           `slot`: per chunk of showings the inputs go up once, the commit, quotient and open phases run back to back with
 *           the range transcript's c and rho and the DLEQ transcript's c_dleq derived between them, the responses
 *           s = nonce - c_dleq * secret follow, and the proof comes down once.
 * openings, rand: as for cg_range_commit_batch; the randomness is the caller's, in the same order.
 * ped_com:  n x 64 B ark-serialize uncompressed: `ped_open.c` (dlog.rs:24-29), which the reference takes as given and the
 *           DLEQ's transcript absorbs as y_0.  One that fails ark's checked G1 deserialisation makes its showing
 *           CG_SHOW_MALFORMED.
 * com_f, com_g, com_q, evals, proofs, pok_c, pok_s: the fields of a `RangeProof` in the layouts cg_range_verify_batch
 *           takes, which are the layouts the three calls and cg_range_respond_batch write: the same bytes as that path
 *           gives for the same openings, rand and challenges.
 * challenges_out: n x 3 x 32 B canonical Fr: c_dleq, c, rho; may be NULL.
 * status:   n x CG_SHOW_MADE / CG_SHOW_MALFORMED.  CG_SHOW_MADE only if every phase made the showing; a malformed
 *           showing (the conditions of the three calls, or a bad ped_com) has zero bytes in EVERY output row and leaves
 *           its neighbours alone.
 * Argument errors are reported before any HIP call; n = 0 is CG_OK; calls on one handle serialise.
 * cg_range_pk_last_kernel_ms reads zeros after this call: its stages interleave. */
int cg_range_prove_batch(cg_range_pk* k, uint32_t slot, const uint8_t* openings, const uint8_t* ped_com, const uint8_t* rand,
                         uint64_t n, uint8_t* com_f, uint8_t* com_g, uint8_t* com_q, uint8_t* evals, uint8_t* proofs,
                         uint8_t* pok_c, uint8_t* pok_s, uint8_t* challenges_out, uint8_t* status);
/* Replaces: `RangeProof::verify_n_bits` (rangeproof.rs:342-424) whole: cg_range_verify_batch without c, rho and k_out.
 *           c and rho are derived on the device from com_f, com_g, com_q as their bytes compress; behind the pairing the
 *           DLEQ's challenge is recomputed from the slot's bases, k_0, ped_com, com_f_basis, k_1 and com_f and compared
 *           with pok_c (dlog.rs:130-174).
 * pok_c is required.  verdicts: CG_VERIFY_ACCEPT exactly where `verify_n_bits(..) == true`: where cg_range_verify_batch
 * accepts AND the recomputed challenge equals pok_c; CG_VERIFY_MALFORMED as there, per showing; else CG_VERIFY_REJECT.
 * The handle's latency mode is honoured, with identical verdicts.  Argument errors, n = 0, chunking and the lock are as
 * for cg_range_verify_batch. */
int cg_range_verify_proofs_batch(cg_range_vk* k, uint32_t slot, const uint8_t* ped_com, const uint8_t* com_f, const uint8_t* com_g,
                                 const uint8_t* com_q, const uint8_t* evals, const uint8_t* proofs, const uint8_t* randomizers,
                                 const uint8_t* pok_c, const uint8_t* pok_s, uint64_t n, uint8_t* verdicts);
/* Replaces: the transcript of `DLogPoK::prove` / `DLogPoK::verify` (dlog.rs:56-58, 77-99; :130-132, 147-169) for n
 *           showings of one shape: `Transcript::new(&[0u8])`, b"context string", then per statement b"num_bases", its
 *           bases under b"base", b"k" and b"y", and the 31-byte challenge.  For hosts without Merlin (INTEGRATION.md,
 *           "Hosts without Merlin"): between cg_show_commit_batch and cg_show_respond_batch, behind cg_verify_show_batch
 *           and cg_range_verify_batch, and for the DLEQ of the three-call range path.  Host only, on the library's worker
 *           threads: no handle, no HIP call, usable in a process without a GPU.
 * Operands come in the forms the other entries hand them out:
 * context:  context_len bytes; context_stride = 0: one context for the whole batch, otherwise showing i's starts at
 *           context + i * context_stride; NULL with length 0 is `None`, which the reference absorbs as the empty string.
 * n_bases:  n_statements counts; bases: the sum of them points, shared by the batch, 64 B ark-serialize uncompressed each
 *           as they lie in a verifying key, statement by statement.
 * k:        n x n_statements x 32 B ark-serialize COMPRESSED, the k_out / ts_out layout.
 * y_head:   n x (n_statements - 1) x 64 B uncompressed: `committed` of a showing, ped_com of a range proof; may be NULL
 *           with one statement.  y_last: n x 64 B: com_hidden of a showing, com_f of a range proof.
 * c_out:    n x 32 B canonical Fr (the top byte is 0).
 * The points are compressed here.  A coordinate >= q or invalid point flags are CG_ERR_INVALID_ARGUMENT naming the base
 * or the showing, and nothing is written; whether a point is on the curve is for the verifying calls to say. */
int cg_dlog_challenge_batch(const uint8_t* context, uint64_t context_len, uint64_t context_stride, uint32_t n_statements,
                            const uint32_t* n_bases, const uint8_t* bases, const uint8_t* k, const uint8_t* y_head,
                            const uint8_t* y_last, uint64_t n, uint8_t* c_out);

/* Verifying whole showings.  The reference's `verify_show` (creds/src/lib.rs:531-700; `verify_show_mdl`, :723-) is more
 * than `ShowGroth16::verify` and `ShowRange::verify`: a range proof is checked against a committed input of the showing
 * SHIFTED by a public value (lib.rs:645-646, :847-848, :868-876),
 *     ped_com = show_groth16.commited_inputs[j] - gamma_abc_g1[pos] * t        (t = cur_time, or days_to_be_age(age)),
 * and the showing is sound only if the range proof speaks about that point.  The two entries below compute the link on
 * the GPU, on the verifying and on the creating side ("Verifying whole showings").
 *
 * One range proof of a showing: which committed input it is about, and the slot of `rk` registered for
 * (gamma_abc_g1[pos], delta_g1) of that input - the vk's entry of the input, i.e. gamma_abc_g1[input index + 1]. */
typedef struct cg_show_range_link {
    uint32_t committed_index;  /* which committed input, counted in committed order (0 = first) */
    uint32_t slot;             /* cg_range_vk_add_bases' slot for that input's bases (cg_range_pk_add_bases' when creating) */
} cg_show_range_link;
/* One range proof per showing, n rows each, in the layouts of cg_range_verify_proofs_batch. */
typedef struct cg_range_rows {
    const uint8_t *com_f, *com_g, *com_q, *evals, *proofs, *randomizers, *pok_c, *pok_s;
} cg_range_rows;
/* Replaces: the cryptographic checks of `verify_show` / `verify_show_mdl` for n showings of one layout in ONE call:
 *           `ShowGroth16::verify` whole (lib.rs:630, :832; groth16rand.rs:232-306 with the DLogPoK's transcript and
 *           `c == self.c`, dlog.rs:130-174), the link above per range proof (lib.rs:645-646, :847-848, :868-876) and
 *           `ShowRange::verify` whole per range proof (lib.rs:650, :852, :881).  Per chunk of showings everything runs
 *           on the device and nothing comes down between the steps: the kernels of cg_verify_show_batch; the DLogPoK's
 *           Merlin transcript over the compressed bases, the recomputed k_i and y_i as their bytes stand, compared with
 *           pok_c; ped_com per (showing, range) from the key's tables, written to device memory that the kernels of
 *           cg_range_verify_proofs_batch then read on the range key's stream, ordered behind the link by an event.
 * NOT done here: the SHA-256 of revealed preimages (lib.rs:560-605), which cg_revealed_digest_batch computes on the host; the
 * freshness test on cur_time (:637-643); and the device proof, whose BN254 half cg_device_link_verify_batch verifies on the
 * same `committed` array and whose Spartan proof over T-256 stays with the host.
 * io_types .. pok_s: as for cg_verify_show_batch; pok_c and pok_s are required.
 * context: the DLogPoK's context string as cg_dlog_challenge_batch takes it: context_len bytes, context_stride = 0 for one
 *          context shared by the batch, otherwise showing i's starts at context + i * context_stride; NULL with length 0 is
 *          `None`.
 * links:   n_ranges of them, shared by the batch.  shifts: n x n_ranges x 32 B canonical Fr, the t of each link.
 * ranges:  n_ranges cg_range_rows of n rows each.  n_ranges = 0 is `ShowGroth16::verify` whole (rk may then be NULL).
 * verdicts:      n x CG_VERIFY_*: MALFORMED if any part is MALFORMED, ACCEPT if every part is ACCEPT, else REJECT.
 * part_verdicts: n x (1 + n_ranges), may be NULL: the Groth16 part first - ACCEPT only where the pairing accepts AND the
 *          recomputed challenge equals pok_c, i.e. `ShowGroth16::verify == true` -, then each range part as
 *          cg_range_verify_proofs_batch answers for the linked ped_com.  A shift >= r or a committed point that fails
 *          the checked deserialisation makes that range part MALFORMED (the latter also the Groth16 part).  ped_com = O is
 *          legal.  A bad showing leaves its neighbours untouched.
 * Errors, all reported before any HIP call and with no output touched: a null array; n_io != cg_pvk_num_inputs
 * (CG_ERR_MALFORMED_KEY); the two handles on different devices; a committed_index >= n_committed; an unknown slot; a slot
 * whose registered 128 bytes are not byte for byte gamma_abc_g1[pos] ‖ delta_g1 of this key for the linked input; a
 * context_stride shorter than context_len.  n = 0 is CG_OK.
 * Locks: both handles' locks are held for the call, always taken in the order cg_pvk, then cg_range_vk.  The latency mode of
 * each handle is honoured, with identical verdicts.  The two halves of a chunk run side by side on the two handles' streams
 * (cg_pvk_set_showings_overlap), which takes about the longer half instead of the sum.  Measured on an MI355X at 26 inputs
 * with one 32-bit range proof (profiles/showing_verify.md): 70 ms for 1024 whole showings and 84 ms for 16384, against 116
 * and 133 ms for cg_verify_show_batch, cg_dlog_challenge_batch and cg_range_verify_proofs_batch in turn; a lone showing
 * with both handles in latency mode 27 ms against 52 ms.  cg_pvk_last_kernel_ms and cg_range_vk_last_kernel_ms read zeros
 * after this call. */
int cg_verify_showings_batch(cg_pvk* k, cg_range_vk* rk, const uint8_t* io_types, uint64_t n_io, const uint8_t* context,
                             uint64_t context_len, uint64_t context_stride, const uint8_t* revealed, const uint8_t* rand_proofs,
                             const uint8_t* com_hidden, const uint8_t* committed, const uint8_t* pok_c, const uint8_t* pok_s,
                             uint32_t n_ranges, const cg_show_range_link* links, const uint8_t* shifts, const cg_range_rows* ranges,
                             uint64_t n, uint8_t* verdicts, uint8_t* part_verdicts);
/* Diagnostic: how cg_verify_showings_batch and cg_create_showings_batch order the two halves of a chunk.  1 = the range
 * half starts on the range key's stream as soon as the link is written, beside the Groth16 half; 0 = it starts when the
 * Groth16 half has finished.  The bytes are the same either way (profiles/showing_verify.md and profiles/showing_create.md
 * have both timings).  A value other than 0 or 1, or a null handle,
 * is CG_ERR_INVALID_ARGUMENT.  (No counterpart in the reference.) */
int cg_pvk_set_showings_overlap(cg_pvk* k, int32_t on);
/* One range proof per showing, n rows each, in the layouts cg_range_prove_batch writes; challenges may be NULL. */
typedef struct cg_range_made { uint8_t *com_f, *com_g, *com_q, *evals, *proofs, *pok_c, *pok_s, *challenges; } cg_range_made;
/* Replaces: the curve arithmetic and the transcripts of `create_show_proof` / `create_show_proof_mdl` (creds/src/lib.rs:364-373,
 *           :468-471, :505-509) for n client states of one layout in ONE call: `ClientState::show_groth16` whole
 *           (groth16rand.rs:100-187, with `DLogPoK::prove`'s Merlin transcript, dlog.rs:56-99, and its responses), per range
 *           proof the link `com.m -= t; com.c -= bases[0] * t` (lib.rs:370-372) and `show_range` whole about it.  It is
 *           cg_show_commit_batch, cg_dlog_challenge_batch over the key's bases, cg_show_respond_batch and, per link,
 *           cg_show_shift_batch and cg_range_prove_batch, with every output row byte for byte what that sequence writes for
 *           the same operands - and nothing coming down or going up again in between.
 * NOT done here: drawing randomness (the library draws none), `revealed_preimages`, and the device proof, whose BN254 half
 * cg_device_link_prove_batch makes from this call's `committed` in a call of its own (cg_device_link_verify_batch verifies it).
 * io_types, proofs, inputs, rand: as for cg_show_commit_batch (rand: cg_show_rand_count scalars per showing, same order).
 * context: as for cg_verify_showings_batch, with the same limits and errors.
 * links:   n_ranges of them, shared by the batch; `slot` is a slot of the PROVING range key rk (cg_range_pk_add_bases).  Two
 *          links may name the same committed input (mDL proves two ranges about one date, with different shifts).
 * shifts:  n x n_ranges x 32 B canonical Fr.  range_rand: n x n_ranges x CG_RANGE_N_RAND x 32 B, the 18 scalars of
 *          cg_range_prove_batch per (showing, link).
 * The opening of link j is no input: it is the showing's own, m = inputs[pos] of the linked committed input and r = that
 * input's r_i in rand (index 2 + committed_index) - `committed_input_openings[ci]` of groth16rand.rs:135-139.
 * rand_proofs, com_hidden, committed: the layouts of cg_show_commit_batch;  pok_c: n x 32 B;  pok_s: n x n_resp x 32 B, the
 * layout of cg_show_respond_batch.  ranges: n_ranges cg_range_made of n rows each.
 * part_status: n x (1 + n_ranges) of CG_SHOW_MADE / CG_SHOW_MALFORMED, may be NULL: the Groth16 part, then the range parts.
 * status:  n x CG_SHOW_*: MADE only if every part of the showing is.
 * A malformed part has zero bytes in each of its rows.  A range part whose Groth16 part is malformed is malformed too: there
 * is no commitment to link from.  A range part alone fails on a shift >= r, a range_rand scalar >= r, or m - t outside
 * [0, 2^n_bits); the Groth16 rows of that showing stay as made.  A bad showing leaves its neighbours untouched.
 * Errors, all reported before any HIP call and with no output touched: a null array (rk, links, shifts, range_rand and
 * ranges may be NULL only with n_ranges = 0, which is `show_groth16` whole); n_io != cg_pvk_num_inputs (CG_ERR_MALFORMED_KEY);
 * an io byte above 2; a key that is not gamma = 1 (CG_ERR_MALFORMED_KEY); the two handles on different devices; a
 * committed_index >= n_committed; an unknown slot; a slot whose registered 128 bytes are not byte for byte gamma_abc_g1[pos] ‖
 * delta_g1 of this key for the linked input; a context_stride shorter than context_len.  n = 0 is CG_OK.
 * Locks: both handles' locks are held for the call, always taken in the order cg_pvk, then cg_range_pk.  The range proofs
 * need the committed points alone, so they run on the range key's stream beside the re-randomisation's long chains when
 * cg_pvk_set_showings_overlap says so; the bytes are the same either way.  Measured on an MI355X at 26 inputs with one 32-bit
 * range proof (profiles/showing_create.md): 17.5 ms for 1024 whole showings and 64 ms for 16384, against 27 and 92 ms for the
 * five separate calls; a lone showing 18 ms against 28 ms.
 * cg_pvk_last_kernel_ms and cg_range_pk_last_kernel_ms read zeros after this call. */
int cg_create_showings_batch(cg_pvk* k, cg_range_pk* rk, const uint8_t* io_types, uint64_t n_io,
                             const uint8_t* context, uint64_t context_len, uint64_t context_stride,
                             const uint8_t* proofs, const uint8_t* inputs, const uint8_t* rand,
                             uint32_t n_ranges, const cg_show_range_link* links, const uint8_t* shifts, const uint8_t* range_rand,
                             uint64_t n,
                             uint8_t* rand_proofs, uint8_t* com_hidden, uint8_t* committed, uint8_t* pok_c, uint8_t* pok_s,
                             const cg_range_made* ranges, uint8_t* status, uint8_t* part_status);
/* Replaces: the creating side's link, `com.m -= t; com.c -= bases[0] * t` before `show_range` (lib.rs:370-372, :468-470,
 *           :505-507), for n openings of the committed input `input_index` (an index into io_types; its base is
 *           gamma_abc_g1[input_index + 1]).
 * openings:    n x 2 x 32 B canonical Fr: m and r (dlog.rs:24-29);  commitments: n x 64 B ark-serialize uncompressed, the
 *              committed point of each showing;  shifts: n x 32 B canonical Fr.
 * openings_out: n x 2 x 32 B: m - t mod r (m < t wraps), and r unchanged;  ped_com_out: n x 64 B: c - t * base (O where
 *              they cancel), both in the layouts cg_range_prove_batch takes.  m - t >= 2^n_bits stays that call's to refuse.
 * status:      n x CG_SHOW_MADE / CG_SHOW_MALFORMED (that row only, its output rows zero bytes): m, r or t >= r, or a
 *              commitment that fails ark's checked G1 deserialisation.
 * input_index >= cg_pvk_num_inputs or a null array is CG_ERR_INVALID_ARGUMENT, reported before any HIP call; n = 0 is CG_OK. */
int cg_show_shift_batch(cg_pvk* k, uint32_t input_index, const uint8_t* openings, const uint8_t* commitments, const uint8_t* shifts,
                        uint64_t n, uint8_t* openings_out, uint8_t* ped_com_out, uint8_t* status);

/* Device-bound showings.  Two of the reference's credential configurations (`mdl1`, `rs256-db`) are "device_bound": after
 * `ShowGroth16::verify`, `verify_show` and `verify_show_mdl` call `DeviceProof::verify` on every showing.
 *
 * One device proof per showing, n rows each. */
typedef struct cg_device_link_rows {
    const uint8_t *com1;    /* n x 64 B ark-serialize uncompressed: DeviceProof.com1, the re-committed com1 */
    const uint8_t *comz;    /* n x 64 B */
    const uint8_t *h_q;     /* n x h_len bytes; may be NULL with h_len = 0 */
    const uint8_t *m;       /* n x 32 B canonical Fr */
    const uint8_t *pi0_c, *pi0_s;   /* n x 32 B;  n x 4 x 32 B: s[0][0], s[0][1], s[1][0], s[1][1] */
    const uint8_t *pi1_c, *pi1_s;   /* n x 32 B;  n x 3 x 32 B: s[0][0], s[1][0], s[1][1] */
} cg_device_link_rows;
/* Replaces: the BN254 half of `DeviceProof::verify` (creds/src/device.rs:168-213), as `verify_show` and `verify_show_mdl` call
 *           it per showing (creds/src/lib.rs:660-680, :893-913), for n showings of one layout in ONE call: pi0 - a DLogPoK
 *           with the equal-scalar pair (0, 0) about com1_orig and the re-committed com1 -, the SHA-256 challenge (e1, e2)
 *           over the text forms of pi0.c, com0, com1 and comz and over h_Q, the recombination
 *           lhs1 = com0 + e1 com1 + e2 comz - m g, and pi1 about lhs1 and comz, both with their Merlin transcripts.  Per
 *           chunk of showings everything runs on the device and nothing comes down between the steps.
 * NOT done here: pi2, the Spartan proof over T-256 (`ECDSAProof::verify`, device.rs:215-216).  The host passes m and e_out on
 * to it; a showing is the reference's `true` where this call answers CG_VERIFY_ACCEPT and pi2 verifies (INTEGRATION.md,
 * "Device-bound showings").
 * UNVERIFIED text forms: the digest is taken over `to_string()` of arkworks 0.4 values - a field element as its decimal digits
 * with no leading zero, ZERO AS THE EMPTY STRING; a point as "infinity" or "(x, y)".  arkworks is not available to this
 * project and the reference pins no such string, so these rules are restated from the 0.4 sources and hold until an
 * arkworks-made DeviceProof meets this code; each is one function of csrc/device_link.hpp.
 * io_types: as for cg_verify_show_batch.  pos0, pos1: the input indices of `device_key_0_value` and `device_key_1_value`, as
 *           cg_show_shift_batch's input_index; g = gamma_abc_g1[pos0 + 1], g' = gamma_abc_g1[pos1 + 1], h = delta_g1.
 * committed: the showing's own n x n_committed x 64 B array, exactly as cg_verify_showings_batch takes it: com0 and com1_orig
 *           are read from it at the committed indices of pos0 and pos1, so they cannot fall out of step with the showing.
 * h_len:    bytes of h_Q per row, at most 64 (`compute_hQ` returns the 32 bytes of a P-256 field element).
 * verdicts: n x CG_VERIFY_*.  ACCEPT: pi0's recomputed challenge equals pi0_c, pi0_s[0] == pi0_s[2], and pi1's recomputed
 *           challenge equals pi1_c.  MALFORMED (that row only, its e_out bytes zero, its parts MALFORMED): com0, com1_orig,
 *           com1 or comz fails ark's checked G1 deserialisation, or m, a challenge or a response is >= r.  A point at
 *           infinity is legal.  Else REJECT.  A bad row leaves its neighbours untouched.
 * part_verdicts: n x 2 for (pi0, pi1), may be NULL.
 * e_out:    n x 32 B: the digest, e1_bytes ‖ e2_bytes, written for every row that is not MALFORMED, accepted or not.
 * Errors, all reported before any HIP call and with no output touched: a null array; n_io != cg_pvk_num_inputs
 * (CG_ERR_MALFORMED_KEY); an io byte above 2; pos0 or pos1 out of range, not CG_IO_COMMITTED, or equal; h_len above 64.
 * n = 0 is CG_OK.  There is no pairing here, so the latency mode of the handle has no bearing.  The call runs on the key's
 * stream under its lock, beside nothing: it may follow cg_verify_showings_batch on the same handle at once.
 * Measured on an MI355X in the mDL-like layout with h_Q of 32 bytes (profiles/device_link.md): 7.6 ms for one proof, 7.1 ms for
 * 1024 and 10.8 ms for 16384 (1.5 M proofs/s), an eighth of what cg_verify_showings_batch takes at that size; the chains are
 * 85 % of it. */
int cg_device_link_verify_batch(cg_pvk* k, const uint8_t* io_types, uint64_t n_io, uint32_t pos0, uint32_t pos1,
                                const uint8_t* committed, const cg_device_link_rows* rows, uint32_t h_len, uint64_t n,
                                uint8_t* verdicts, uint8_t* part_verdicts, uint8_t* e_out);
/* Diagnostic: what the four kernels of the handle's last cg_device_link_verify_batch took, by HIP events, summed over its
 * chunks: the digest and scalar stage, the terms, the sums, the two transcripts.  Zeros before the first such call.
 * (No counterpart in the reference.) */
int cg_device_link_last_kernel_ms(cg_pvk* k, float ms[4]);
/* The scalars a device proof draws, in the reference's drawing order (device.rs:104-160): z, t_z (comz = z g + t_z h); r1 (the
 * re-committed com1 = q1 g + r1 h); a, b, d (pi0's nonces: r[0] = [a, b], r[1] = [a, d], the equal-scalar pair (0, 0) applied);
 * n0, n1, n2 (pi1's: r[0] = [n0], r[1] = [n1, n2]). */
#define CG_DEVICE_LINK_N_RAND 9
/* One device proof per showing, n rows each, in exactly the layouts cg_device_link_rows takes: com1, comz n x 64 B
 * ark-serialize uncompressed; m n x 32 B; pi0_c n x 32 B; pi0_s n x 4 x 32 B; pi1_c n x 32 B; pi1_s n x 3 x 32 B. */
typedef struct cg_device_link_made { uint8_t *com1, *comz, *m, *pi0_c, *pi0_s, *pi1_c, *pi1_s; } cg_device_link_made;
/* Replaces: the BN254 half of `DeviceProof::prove` (creds/src/device.rs:104-160) for n showings of one layout in ONE call: comz
 *           and the re-committed com1, pi0 with its Merlin transcript and responses, the SHA-256 challenge (e1, e2), the
 *           recombination m = q0 + q1 e1 + z e2 and r = r0 + r1 e1 + t_z e2, lhs1 and pi1.  The prover knows every discrete
 *           logarithm, so each group element is a sum of walks through the key's fixed-base tables of g, g' and h - lhs1 is the
 *           one walk r h - and a proof has no variable-base chain.  Per chunk of showings everything runs on the device and
 *           nothing comes down between the steps.
 * NOT done here: pi2 (`ECDSAProof::prove`), and in THIS call `compute_hQ`, which is Poseidon over P-256's base field: h_Q is
 * an input here, from cg_hq_batch or from the host.  cg_device_link_prove_hq_batch below computes it on the device in the same
 * call.  The library draws no randomness.  Afterwards the host hands m, e_out and its own z to `ECDSAProof::prove`
 * ("Creating device proofs").
 * UNVERIFIED text forms: as for cg_device_link_verify_batch; both calls take the digest from the same function of
 * csrc/device_link.hpp.
 * io_types, n_io, pos0, pos1, committed, h_q, h_len: exactly as for cg_device_link_verify_batch.  com0 and com1_orig are read
 *           from the showing's own `committed` array at the committed indices of pos0 and pos1.
 * openings: n x 4 x 32 B canonical Fr: q0, r0, q1, r1_orig - `committed_input_openings[1]` and `[2]` of lib.rs:378-379.  For a
 *           showing made by cg_create_showings_batch, m = inputs[pos] and r = rand[2 + committed_index] of that call.
 * rand:     n x CG_DEVICE_LINK_N_RAND x 32 B canonical Fr, in the order above.
 * out:      the proof's rows.  The caller passes h_q itself on to the verifier.
 * e_out:    n x 32 B: the digest, e1_bytes ‖ e2_bytes.
 * status:   n x CG_SHOW_MADE / CG_SHOW_MALFORMED.  MALFORMED means that row only: every output row of it, e_out included, is
 *           zero bytes, and its neighbours are untouched.  A row is malformed when an opening or rand scalar is >= r, when com0
 *           or com1_orig fails ark's checked G1 deserialisation, or when an opening does not open its committed point
 *           (q0 g + r0 h != com0, or q1 g' + r1_orig h != com1_orig; O against the infinity flag counts as equal).  The last
 *           is the library's fail-closed reading of the reference's `assert!(lhs1 == h * r)` (device.rs:153-154), which
 *           panics on a wrong opening of com0; it is extended to com1_orig, where the reference would silently emit a proof
 *           that does not verify.  Zero scalars and points at infinity are legal everywhere: z = t_z = 0 gives comz = O.
 * Errors, all reported before any HIP call and with no output touched: a null array or a null member of `out` (h_q may be NULL
 * only with h_len = 0); n_io != cg_pvk_num_inputs (CG_ERR_MALFORMED_KEY); an io byte above 2; pos0 or pos1 out of range, not
 * CG_IO_COMMITTED, or equal; h_len above 64.  n = 0 is CG_OK.  The call runs on the key's stream under its lock; it has
 * per-call arrays of its own, so it and cg_device_link_verify_batch do not evict each other on one handle.
 * Measured on an MI355X: profiles/device_link_create.md. */
int cg_device_link_prove_batch(cg_pvk* k, const uint8_t* io_types, uint64_t n_io, uint32_t pos0, uint32_t pos1,
                               const uint8_t* committed, const uint8_t* openings, const uint8_t* rand,
                               const uint8_t* h_q, uint32_t h_len, uint64_t n,
                               const cg_device_link_made* out, uint8_t* e_out, uint8_t* status);
/* Diagnostic: what the six kernels of the handle's last cg_device_link_prove_batch took, by HIP events, summed over its
 * chunks: the checks, the fifteen walks, the sums, pi0 with the digest, lhs1, pi1.  Zeros before the first such call.
 * (No counterpart in the reference.) */
int cg_device_link_prove_last_kernel_ms(cg_pvk* k, float ms[6]);
/* Replaces: the Poseidon permutation over P-256's base field (p = 2^256 - 2^224 + 2^192 + 2^96 - 1) that `compute_hQ` is built
 *           on: width 3, (R_F, R_P) = (8, 55), neptune's `Strength::Standard` constants derived by the library itself
 *           (csrc/poseidon_p256.hpp), for n states in one call.  The primitive under cg_hq_batch, and the entry through which
 *           the field's edges are reached.
 * states, out: n x 3 x 32 B, canonical little-endian.
 * status: n x CG_SHOW_MADE / CG_SHOW_MALFORMED.  MALFORMED means that row only: an element of it is >= p, and its output is
 *         zero bytes.
 * Errors, reported before any HIP call and with no output touched: a null argument.  n = 0 is CG_OK.  Runs on the key's stream
 * under its lock; the constants go up to the handle once, with the first call that needs them. */
int cg_poseidon_p256_permute_batch(cg_pvk* k, const uint8_t* states, uint64_t n, uint8_t* out, uint8_t* status);
/* Replaces: `compute_hQ` (ecdsa-pop/src/lib.rs:308-320): h_Q = Poseidon(q0, q1, z) over P-256's base field, for n rows in one
 *           call.
 * UNVERIFIED readings: the constants, the permutation and the IO-pattern tag reproduce neptune's own known answers over
 * BLS12-381's Fr (tests/golden/neptune_kats.json).  Three things no recorded value pins, each one function of
 * csrc/poseidon_p256.hpp, until a Rust-made h_Q meets this code: (1) the Grain LFSR's first byte takes 8 bits where the
 * field's bit length is a multiple of 8, as P-256's 256 is; (2) the sponge is state = [tag, 0, 0], q0 and q1 added to elements
 * 1 and 2, a permutation, z added to element 1, a permutation, element 1 out; (3) `to_bytes()` reversed is the element's 32
 * bytes big-endian.
 * q:       n x 3 x 32 B canonical Fr: q0, q1, z as a showing holds them (r < p, so each is a field element).
 * h_q_out: n x 32 B big-endian: exactly the bytes cg_device_link_rows.h_q and cg_device_link_prove_batch take with h_len = 32.
 * status:  n x CG_SHOW_MADE / CG_SHOW_MALFORMED.  MALFORMED means that row only: a scalar of it is >= r, the rule of the
 *          openings, and its output is zero bytes.
 * Errors and scheduling as for cg_poseidon_p256_permute_batch.  Measured on an MI355X: profiles/device_link_hq.md. */
int cg_hq_batch(cg_pvk* k, const uint8_t* q, uint64_t n, uint8_t* h_q_out, uint8_t* status);
/* cg_device_link_prove_batch with `compute_hQ` in the same call: one more kernel in front of the chunk's six computes h_Q from
 * q0 and q1 (openings) and z (rand[0]) where the digest reads it, so the host computes nothing before the call and hands only
 * m, e_out and z to `ECDSAProof::prove` after it.
 * NOT done here: pi2 (`ECDSAProof::prove`); the library draws no randomness.
 * UNVERIFIED: the text forms of cg_device_link_verify_batch and the three readings of cg_hq_batch.
 * Every argument but the last as for cg_device_link_prove_batch, which has h_q and h_len in addition.
 * h_q_out: n x 32 B: the row's h_Q, which the caller passes on to the verifier.  Every other output is byte for byte what
 *          cg_hq_batch followed by cg_device_link_prove_batch with h_len = 32 writes.  A malformed row has h_q_out zero as well.
 * Errors: as for cg_device_link_prove_batch, and a null h_q_out.  n = 0 is CG_OK. */
int cg_device_link_prove_hq_batch(cg_pvk* k, const uint8_t* io_types, uint64_t n_io, uint32_t pos0, uint32_t pos1,
                                  const uint8_t* committed, const uint8_t* openings, const uint8_t* rand, uint64_t n,
                                  const cg_device_link_made* out, uint8_t* e_out, uint8_t* status, uint8_t* h_q_out);
/* Diagnostic: ms[0] what the kernel of the handle's last cg_hq_batch or cg_poseidon_p256_permute_batch took, ms[1] what the
 * h_Q kernel of its last cg_device_link_prove_hq_batch took (cg_device_link_prove_last_kernel_ms has the six behind it), by
 * HIP events, summed over the chunks; *uploads: how often the Poseidon constants went up to this handle, 0 before the first
 * call that needs them and 1 ever after.  (No counterpart in the reference.) */
int cg_hq_last_kernel_ms(cg_pvk* k, float ms[2], uint32_t* uploads);
/* Replaces: `ECDSACircuitPublicInputs::compute_TU` (ecdsa-pop/src/lib.rs:217-240), which a relying party runs at the top of
 *           `ECDSAProof::verify`: from the proof's R = (r_x, r_y) and the digest, T = r^-1 · R and U = (-d · r^-1) · G on P-256,
 *           with r = R.x mod n and d = digest mod n - the public inputs of pi2's circuit - for n rows in one call.  P-256 group
 *           arithmetic only (csrc/p256.hpp over csrc/fp256.hpp and csrc/fq256.hpp); nothing of the key is used, the handle
 *           lends its stream, its lock and a state slot.
 * NOT done here: pi2 itself (Spartan over T-256).  The host hands T and U to its verifier.
 * Every P-256 quantity is 32 bytes BIG-endian, the convention of h_Q, of SEC1 and of the 64-byte signature
 * `ECDSASig::new_from_bytes` splits; a point is x ‖ y, 64 B, and the identity is 64 zero bytes, which is what halo2curves'
 * `to_affine` makes of it.
 * r_xy:   n x 64 B: R.    digest: n x 32 B, read as the reference's `from_str_vartime` reads it: an integer below 2^256,
 *         reduced mod n.
 * t_xy, u_xy: n x 64 B.  d = 0 mod n is valid: U is then the identity, 64 zero bytes, and the status CG_SHOW_MADE.
 * status: n x CG_SHOW_MADE / CG_SHOW_MALFORMED.  MALFORMED means that row only, with every output of it zero bytes: a
 *         coordinate of R is >= p (the reference reduces it silently; this library fails closed on non-canonical input, as it
 *         does for scalars >= r), R is not on the curve (the reference panics on `from_xy(..).unwrap()`), or r = 0 mod n (the
 *         reference asserts).
 * Errors, reported before any HIP call and with no output touched: a null argument.  n = 0 is CG_OK.  Runs on the key's stream
 * under its lock, in chunks; the table of G (0.5 MB) goes up to the handle once, with the first call that needs it.
 * A kernel's time is one lane's latency at every batch size, some milliseconds: a host with one row and a P-256 library of
 * its own should use that.  Measured on an MI355X: profiles/p256_tu.md. */
int cg_p256_tu_batch(cg_pvk* k, const uint8_t* r_xy, const uint8_t* digest, uint64_t n, uint8_t* t_xy, uint8_t* u_xy, uint8_t* status);
/* Replaces: `compute_RTU` (ecdsa-pop/src/lib.rs:180-215), which a prover runs at the top of `ECDSAProof::prove` and which is
 *           the only place where the device's ECDSA signature is checked: R = (d/s) · G + (r/s) · Q, R.x mod n must equal r,
 *           and then T and U as cg_p256_tu_batch makes them from R, for n rows in one call.  The sum goes through a complete
 *           addition: a signer chooses Q, and where Q is a small multiple of +-G the two products coincide or cancel.
 * q_xy:   n x 64 B: the device's public key.    sig: n x 64 B: r ‖ s.    digest: n x 32 B.    Byte forms as above.
 * r_xy, t_xy, u_xy: n x 64 B.  Feeding r_xy and digest to cg_p256_tu_batch returns the same t_xy and u_xy.
 * status: n x CG_SHOW_MADE / CG_SHOW_MALFORMED / CG_P256_BAD_SIGNATURE, that row only, with every output of a row that is not
 *         MADE zero bytes.  MALFORMED: Q fails the checks of R above, or r or s is outside [1, n - 1].  BAD_SIGNATURE: R is
 *         the identity or R.x mod n != r (the reference panics on its assertion).
 * Errors and scheduling as for cg_p256_tu_batch. */
int cg_p256_rtu_batch(cg_pvk* k, const uint8_t* q_xy, const uint8_t* sig, const uint8_t* digest, uint64_t n, uint8_t* r_xy, uint8_t* t_xy,
                      uint8_t* u_xy, uint8_t* status);
/* Diagnostic: what the three kernels of the handle's last cg_p256_tu_batch or cg_p256_rtu_batch took - the scalar stage, the
 * terms, the finishing stage - by HIP events, summed over the chunks; *uploads: how often the table of G went up to this
 * handle, 0 before the first call that needs it and 1 ever after.  (No counterpart in the reference.) */
int cg_p256_last_kernel_ms(cg_pvk* k, float ms[3], uint32_t* uploads);

/* ---- pi2's witness commitment: the group T-256 and Hyrax rows ----------------------------------------------------------------
 * T-256 (forks/halo2curves/src/t256/) is the group every commitment of `spartan_t256` lives in: y^2 = x^3 - 3x + b over the
 * prime p_T of t256/fp.rs:10, of prime order q = P-256's base prime (csrc/t256.hpp over csrc/ft256.hpp).
 * Byte forms, as halo2curves writes them (serde.rs:174-319, src/derive/curve.rs:69-73 and :139-181,
 * derive/src/field/mod.rs:326-344 and :470-476).  UNVERIFIED: the reference pins no T-256 bytes (t256/curve.rs:129 says so
 * itself), so these are readings of its code that no byte made by it has confirmed; each has one reader or writer in
 * csrc/t256.hpp and one in tests/t256_vectors.py.
 *   a coordinate       32 B big-endian
 *   a scalar           32 B little-endian, below q: the form cg_poseidon_p256_permute_batch takes for the same field
 *   uncompressed point x ‖ y, 64 B; the identity is 64 zero bytes
 *   compressed point   33 B: byte 0 has bit 7 set when y is odd and bit 6 set for the identity (whose bit 7 is clear),
 *                      bytes 1..33 are x big-endian; the identity is 0x40 and 32 zero bytes */
typedef struct cg_t256_gens cg_t256_gens;
/* Replaces: what `MultiCommitGens { G, h }` (forks/Spartan-t256/src/commitments.rs) is to the commitments below: a set of
 *           n_gens generators and the blinding generator h, held as fixed-base tables (8-bit windows, 522 240 B a point) that
 *           are built on the host and stay on the current device.
 * NOT done here: `MultiCommitGens::new` (SHAKE-256 and hash-to-curve), which stays on the host; the host hands over the points.
 * g_xy: n_gens x 64 B, h_xy: 64 B, uncompressed points (UNVERIFIED byte form, above).
 * Errors, all reported before any HIP call: a null argument; n_gens < 1 or so large that the n_gens + 1 tables pass 1 GiB
 * (n_gens > 2055; 257 tables are 134 MB); a coordinate >= p_T (the reference reduces it silently; this library fails closed on
 * non-canonical input); a point off the curve; the identity - each CG_ERR_INVALID_ARGUMENT, naming the point. */
int cg_t256_gens_load(const uint8_t* g_xy, uint64_t n_gens, const uint8_t* h_xy, cg_t256_gens** out);
void cg_t256_gens_free(cg_t256_gens* g);
/* *n_gens as loaded, *table_bytes what the set's tables take on the device.  (No counterpart in the reference.) */
int cg_t256_gens_info(const cg_t256_gens* g, uint64_t* n_gens, uint64_t* table_bytes);
/* Replaces: `Vec<Scalar>::commit` (forks/Spartan-t256/src/commitments.rs:88-99) for n_rows rows over one set of generators:
 *           row i is sum_j scalars[i][j] · G[j] + blinds[i] · h, written compressed (UNVERIFIED byte form, above).  The row
 *           length is the set's n_gens - the reference asserts equality -; with n_gens = 1 this is `Scalar::commit` (:81-86).
 * scalars: n_rows x n_gens x 32 B.    blinds: n_rows x 32 B.    out33: n_rows x 33 B.
 * status: n_rows x CG_SHOW_MADE / CG_SHOW_MALFORMED.  MALFORMED means that row only, its 33 bytes zero: a scalar of the row or
 *         its blind is >= q.  A row whose sum is the identity is MADE, and 0x40 with 32 zero bytes.
 * Errors, reported before any HIP call and with no output touched: a null argument.  n_rows = 0 is CG_OK.  The library draws
 * no randomness: the blinds are the caller's, from its `RandomTape`.  Runs on the handle's stream under its lock, in chunks of
 * at most 16384 rows and 64 MB of scalars; a chunk of cg_hyrax_commit_batch holds whole proofs and never less than one, so at
 * num_vars = 22, the one shape whose proof is larger (2^22 scalars), it is that proof's 128 MB.  Measured on an MI355X: profiles/t256_commit.md. */
int cg_t256_commit_rows_batch(cg_t256_gens* g, const uint8_t* scalars, const uint8_t* blinds, uint64_t n_rows, uint8_t* out33,
                              uint8_t* status);
/* Replaces: `DensePolynomial::commit` (forks/Spartan-t256/src/dense_mlpoly.rs:181-206, `commit_inner` :151-163), the first
 *           step of `R1CSProof::prove` (r1csproof.rs:163-173), for n proofs: the 2^num_vars evaluations as an L x R matrix,
 *           L = 2^(num_vars / 2) and R = 2^(num_vars - num_vars / 2) (`compute_factored_lens`, :88-90), and one commitment per
 *           row - the kernels of cg_t256_commit_rows_batch on n · L rows, which writes the same bytes for the same data.
 * NOT done here: the rest of pi2 - the sum-checks, the dot-product and evaluation proofs, the verifier.
 * vars: n x 2^num_vars x 32 B.    blinds: n x L x 32 B.    out33: n x L x 33 B, in the order `PolyCommitment.C` has
 * (UNVERIFIED byte form, above).
 * status: n x CG_SHOW_MADE / CG_SHOW_MALFORMED, one per PROOF: a scalar or blind of the proof is >= q, and all its L rows are
 *         zero bytes; no other proof is touched.
 * Errors, reported before any HIP call and with no output touched: a null argument; R != the set's n_gens.  n = 0 is CG_OK.
 * Scheduling as for cg_t256_commit_rows_batch; a chunk holds whole proofs. */
int cg_hyrax_commit_batch(cg_t256_gens* g, uint32_t num_vars, const uint8_t* vars, const uint8_t* blinds, uint64_t n, uint8_t* out33,
                          uint8_t* status);
/* Diagnostic: what the kernels of the handle's last cg_t256_commit_rows_batch or cg_hyrax_commit_batch took - ms[0] the check
 * of the scalars, ms[1] the group stage (the rows' sums and their normalisation) - by HIP events, summed over the chunks; *lanes_per_row: how many lanes shared a row in its
 * last chunk (csrc/t256commit.hip has the rule), 0 before the first call.  (No counterpart in the reference.) */
int cg_t256_commit_last_kernel_ms(cg_t256_gens* g, float ms[2], uint32_t* lanes_per_row);
/* Replaces: the digests of `revealed_preimages` that `verify_show` places among the public inputs (creds/src/lib.rs:590-603):
 *           per hashed attribute SHA-256 of the preimage string and its first 31 bytes through `bits_to_num`
 *           (creds/src/utils.rs:78-94), as the canonical Fr a host places into `revealed`.  Host only, on the library's worker
 *           threads: no handle, no HIP call, usable in a process without a GPU.
 * Item i is data[offsets[i] .. offsets[i+1]); offsets has n_items + 1 entries, ascending; an item has fewer than 2^32 bytes.
 * out: n_items x 32 B, little-endian: byte j < 31 is digest byte j with its bits mirrored, byte 31 is zero. */
int cg_revealed_digest_batch(const uint8_t* data, const uint64_t* offsets, uint64_t n_items, uint8_t* out);

/* Replaces: `prepare_verifying_key` (forks/groth16/src/verifier.rs:13-20), on the host (one pairing).
 * vk_bytes: one VerifyingKey as ark-serialize writes it (the fork's layout, delta_g1 included); pvk_out receives the
 * PreparedVerifyingKey bytes (*len of them; pvk_out = NULL only reports *len).  A buffer shorter than *len is
 * CG_ERR_INVALID_ARGUMENT. */
int cg_prepare_verifying_key(const uint8_t* vk_bytes, uint64_t vk_len, uint8_t* pvk_out, uint64_t cap, uint64_t* len);

/* Diagnostic: the shader clock (GHz) the GPU holds over the next `window_us` microseconds, measured on the device by
 * one wave that compares the shader-cycle counter with the constant-rate counter - callable from a second thread while
 * proofs run, which is how bench.py reports the clock its peaks should be scaled by.  device -1 = current.
 * (No counterpart in the reference: CPU provers do not report their clock either.) */
int cg_probe_shader_clock(int32_t device, uint32_t window_us, double* ghz_out);

/* Library / device description for logs ("crescent_gpu 0.1 gfx950 ..."). */
const char* cg_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CRESCENT_GPU_H */
