// The BN254 half of a device proof made on the GPU: `DeviceProof::prove` (creds/src/device.rs:104-160) short of `compute_hQ`
// and of pi2 (`ECDSAProof::prove`), for a batch of device-bound showings under one cg_pvk.  The creating side of what
// csrc/devicelink.hip verifies; the arithmetic and the enumerations are csrc/device_link_make.hpp's.
//
// The prover knows every discrete logarithm, so a proof has no variable-base chain: sixteen walks through the key's 8-bit
// tables of g = gamma_abc_g1[pos0 + 1], g' = gamma_abc_g1[pos1 + 1] and h = delta_g1, fifteen of which depend on no challenge.
// A chunk of proofs runs six kernels on the key's own non-blocking stream, under its lock, with nothing coming down in
// between; partials are laid out TERM-MAJOR within the chunk (term t of proof p at t·m + p), so that a wave walks one table:
//   k_dlm_check   one lane per proof: the 13 scalars below r, ark's checked deserialisation of com0 and com1_orig -> a flag byte
//   k_dlm_terms   one lane per (term, proof): the fifteen walks                                              -> XYZZ partials
//   k_dlm_sum     one lane per (sum, proof): the eight sums by the general `add` - chosen rows make partials coincide or
//                 cancel.  Six are normalised: com1 and comz go out as ark-serialize's uncompressed bytes, and they and the
//                 four k as compressed bytes into the proof's row of transcript points.  The two opening checks compare
//                 q0 g + r0 h with com0 and q1 g' + r1_orig h with com1_orig in projective form      -> a byte per check
//   k_dlm_pi0     one lane per proof: the status byte; pi0's transcript (the sponge in LDS) -> c0; pi0's responses; the digest
//                 of the message (the SHA block and a coordinate's digits in the same LDS, the sponge being done) -> e_out; m, and
//                 r = r0 + r1 e1 + t_z e2, which stays on the device.  A malformed proof has every output row zeroed here.
//   k_dlm_lhs1    one lane per proof: lhs1 = r h, one walk, normalised and compressed (r = 0 gives O)
//   k_dlm_pi1     one lane per proof: pi1's transcript over y = (lhs1, comz) -> c1; pi1's responses
// A malformed proof costs nothing after the stage that found it.  k_dlm_pi0 and k_dlm_pi1 do arithmetic on bytes and words
// only and declare no private segment.
//
// h_Q (`compute_hQ`, ecdsa-pop/src/lib.rs:308-320) is csrc/poseidon_p256.hpp's, one lane per hash, on the same stream under the
// same lock: k_hq_permute behind cg_poseidon_p256_permute_batch, k_hq_hash behind cg_hq_batch, and k_hq_link, which
// cg_device_link_prove_hq_batch runs in front of the six kernels above to fill the chunk's h_Q rows from the openings
// (q0, q1) and rand[0] (z), so that k_dlm_pi0's digest finds them on the device.  The Poseidon constants are derived on the
// host once per process and uploaded once per handle.  The three kernels keep their state in registers, read the constants
// at a wave-uniform address and declare no private segment.
#include <memory>

#include "common.hpp"
#include "device_link_make.hpp"
#include "fixed_base.hpp"
#include "key_handle.hpp"
#include "poseidon_p256.hpp"

using namespace cg;

namespace {

constexpr uint64_t DLMCHUNK = 1u << 15;    // proofs per launch set; 3 KB of device memory per proof
constexpr int DLMBLOCK = 64;
static_assert(ML_STATE >= SHA_BLOCK + DL_DIGITS_ROOM, "the digest's block and digits take the sponge's place");

// one chunk's arrays on the device, as the caller laid them out
struct DlmArgs {
    const uint32_t* committed;             // n_com x 16 words per proof; com0 at ci0, com1_orig at ci1
    uint32_t n_com, ci0, ci1;
    const uint32_t *openings, *rand;       // DLM_N_OPEN and DLM_N_RAND scalars of 8 words per proof
    const uint8_t* h_q;                    // h_len bytes per proof
    uint32_t h_len;
    uint64_t n;
    __device__ const uint32_t* com0(uint64_t p) const { return committed + 16 * (p * n_com + ci0); }
    __device__ const uint32_t* com1_orig(uint64_t p) const { return committed + 16 * (p * n_com + ci1); }
    __device__ const uint32_t* open(uint64_t p) const { return openings + 8 * DLM_N_OPEN * p; }
    __device__ const uint32_t* rnd(uint64_t p) const { return rand + 8 * DLM_N_RAND * p; }
};
// one chunk's output rows on the device: 16, 16, 8, 8, 32, 8, 24 and 8 words per proof, and the status byte
struct DlmOut {
    uint32_t *com1, *comz, *m, *pi0_c, *pi0_s, *pi1_c, *pi1_s, *e;
    uint8_t* status;
};

__global__ __launch_bounds__(DLMBLOCK) void k_dlm_check(DlmArgs a, uint8_t* __restrict__ flags) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    bool ok = dlm_in_range(a.open(p), a.rnd(p));
    (void)dev_g1(a.com0(p), ok);
    (void)dev_g1(a.com1_orig(p), ok);
    flags[p] = ok ? 0 : (uint8_t)DL_MALFORMED;
}

__global__ __launch_bounds__(DLMBLOCK) void k_dlm_terms(DlmArgs a, const uint8_t* __restrict__ flags, const G1Affine* __restrict__ tab_g,
                                                       const G1Affine* __restrict__ tab_gp, const G1Affine* __restrict__ tab_h,
                                                       G1XYZZ* __restrict__ part) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t m = a.n;
    if (g >= m * DLM_N_TERMS) return;
    const uint32_t t = (uint32_t)(g / m);
    const uint64_t p = g % m;
    if (flags[p] & DL_MALFORMED) return;
    const DlmTerm d = dlm_term(t);
    const uint32_t* x = (d.from_rand ? a.rnd(p) : a.open(p)) + 8 * d.index;
    const G1Affine* tb = d.base == DLM_BASE_G ? tab_g : d.base == DLM_BASE_GP ? tab_gp : tab_h;
    part[g] = fixed_base_mul(tb, x);
}

// pts: DLM_N_POINTS x 8 words per proof; opened: a byte per (proof, opening check), 1 where the opening opens its point
__global__ __launch_bounds__(DLMBLOCK) void k_dlm_sum(DlmArgs a, const uint8_t* __restrict__ flags, const G1XYZZ* __restrict__ part,
                                                     uint32_t* __restrict__ com1, uint32_t* __restrict__ comz, uint32_t* __restrict__ pts,
                                                     uint8_t* __restrict__ opened) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t m = a.n;
    if (g >= m * DLM_N_OUT) return;
    const uint32_t o = (uint32_t)(g / m);
    const uint64_t p = g % m;
    if (flags[p] & DL_MALFORMED) return;
    const G1XYZZ sum = dlm_sum(o, [&](uint32_t t) { return part[(uint64_t)t * m + p]; });
    if (o == DLM_O_OPEN0 || o == DLM_O_OPEN1) {
        const G1Affine c = dev_g1_unchecked(o == DLM_O_OPEN0 ? a.com0(p) : a.com1_orig(p));
        opened[2 * p + (o - DLM_O_OPEN0)] = dlm_opens(sum, c) ? 1 : 0;
        return;
    }
    const G1Affine q = to_affine(sum);
    if (o == DLM_O_COM1) dev_put_g1(q, com1 + 16 * p, false);
    if (o == DLM_O_COMZ) dev_put_g1(q, comz + 16 * p, false);
    dev_put_g1(q, pts + 8 * (DLM_N_POINTS * p + dlm_point_of(o)), true);
}

__global__ __launch_bounds__(DLMBLOCK) void k_dlm_pi0(DlmArgs a, const uint8_t* __restrict__ flags, const uint8_t* __restrict__ opened,
                                                     const uint8_t* __restrict__ consts, uint32_t* __restrict__ pts, DlmOut out,
                                                     uint32_t* __restrict__ r) {
    __shared__ __attribute__((aligned(8))) uint8_t lds[DLMBLOCK * ML_STATE];
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    const bool made = !(flags[p] & DL_MALFORMED) && opened[2 * p] && opened[2 * p + 1];
    out.status[p] = made ? CG_SHOW_MADE : CG_SHOW_MALFORMED;
    if (!made) {
        for (int l = 0; l < 16; ++l) out.com1[16 * p + l] = out.comz[16 * p + l] = 0;
        for (int l = 0; l < 8; ++l) out.m[8 * p + l] = out.pi0_c[8 * p + l] = out.pi1_c[8 * p + l] = out.e[8 * p + l] = 0;
        for (int l = 0; l < 32; ++l) out.pi0_s[32 * p + l] = 0;
        for (int l = 0; l < 24; ++l) out.pi1_s[24 * p + l] = 0;
        return;
    }
    uint8_t* mine = lds + ML_STATE * threadIdx.x;
    uint32_t* row = pts + 8 * DLM_N_POINTS * p;
    uint32_t *c0 = out.pi0_c + 8 * p, *e = out.e + 8 * p;
    ml_compress_g1(a.com1_orig(p), row + 8 * DLM_P_COM1_ORIG);
    dlm_challenge(mine, consts, 0u, row, (uint8_t*)c0);
    dlm_pi0_responses(c0, a.open(p), a.rnd(p), out.pi0_s + 32 * p);
    dl_challenge_digest(mine, mine + SHA_BLOCK, c0, a.com0(p), out.com1 + 16 * p, out.comz + 16 * p, a.h_q + p * a.h_len, a.h_len, (uint8_t*)e);
    dlm_recombine(e, a.open(p), a.rnd(p), out.m + 8 * p, r + 8 * p);
}

__global__ __launch_bounds__(DLMBLOCK) void k_dlm_lhs1(uint64_t n, const uint8_t* __restrict__ status, const uint32_t* __restrict__ r,
                                                      const G1Affine* __restrict__ tab_h, uint32_t* __restrict__ pts) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || status[p] != CG_SHOW_MADE) return;
    dev_put_g1(to_affine(fixed_base_mul(tab_h, r + 8 * p)), pts + 8 * (DLM_N_POINTS * p + DLM_P_LHS1), true);
}

__global__ __launch_bounds__(DLMBLOCK) void k_dlm_pi1(DlmArgs a, const uint8_t* __restrict__ consts, const uint32_t* __restrict__ pts,
                                                     const uint32_t* __restrict__ r, DlmOut out) {
    __shared__ __attribute__((aligned(8))) uint8_t sponge[DLMBLOCK * ML_STATE];
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n || out.status[p] != CG_SHOW_MADE) return;
    uint32_t* c1 = out.pi1_c + 8 * p;
    dlm_challenge(sponge + ML_STATE * threadIdx.x, consts, 1u, pts + 8 * DLM_N_POINTS * p, (uint8_t*)c1);
    dlm_pi1_responses(c1, r + 8 * p, a.rnd(p), out.pi1_s + 24 * p);
}

// The per-call arrays of a key's device-link maker: grown to the largest chunk seen, never shrunk; bytes are the caller's.
struct DlmState {
    RowBuf b_comm, b_open{32 * DLM_N_OPEN}, b_rand{32 * DLM_N_RAND}, b_hq;
    RowBuf b_com1{64}, b_comz{64}, b_m{32}, b_c0{32}, b_s0{128}, b_c1{32}, b_s1{96}, b_e{32}, b_status{1};
    RowBuf b_flags{1}, b_opened{2}, b_pts{32 * DLM_N_POINTS}, b_r{32};
    DevBuf<G1XYZZ> b_part;                 // one partial per (term, proof)
    DevBuf<uint8_t> consts;
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // around the six kernels of a chunk
    float ms[6] = {0, 0, 0, 0, 0, 0};                                                        // of the last call, summed over its chunks
    ~DlmState() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
};
void dlm_state_free(void* s) { delete (DlmState*)s; }

// ---- h_Q --------------------------------------------------------------------------------------------------------------------
// states: three canonical elements of P-256's field per row; a row with an element >= p is malformed and comes back zero
__global__ __launch_bounds__(DLMBLOCK) void k_hq_permute(const F256* __restrict__ consts, const uint32_t* __restrict__ states, uint64_t n,
                                                        uint32_t* __restrict__ out, uint8_t* __restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const bool ok = pos_permute_row(consts, states + 24 * p, out + 24 * p);
    if (!ok)
        for (int l = 0; l < 24; ++l) out[24 * p + l] = 0;
    status[p] = ok ? CG_SHOW_MADE : CG_SHOW_MALFORMED;
}

// q: q0, q1 and z per row, canonical Fr; h_q: 32 bytes per row
__global__ __launch_bounds__(DLMBLOCK) void k_hq_hash(const F256* __restrict__ consts, const uint32_t* __restrict__ q, uint64_t n,
                                                     uint32_t* __restrict__ h_q, uint8_t* __restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t* row = q + 24 * p;
    status[p] = pos_hq_row(consts, row, row + 8, row + 16, h_q + 8 * p) ? CG_SHOW_MADE : CG_SHOW_MALFORMED;
}

// the same from a chunk of the maker's inputs; a row with a scalar >= r gets zero bytes and is found malformed by k_dlm_check
__global__ __launch_bounds__(DLMBLOCK) void k_hq_link(const F256* __restrict__ consts, DlmArgs a, uint32_t* __restrict__ h_q) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    (void)pos_hq_row(consts, a.open(p) + 8 * DLM_Q0, a.open(p) + 8 * DLM_Q1, a.rnd(p) + 8 * DLM_Z, h_q + 8 * p);
}

// A key's Poseidon constants on the device, uploaded by the first call that needs them, and the arrays of the two h_Q
// entries.  Its own slot of the handle: the maker's and the verifier's arrays stay where they are.
struct HqState {
    DevBuf<F256> consts;
    uint32_t uploads = 0;
    RowBuf b_in{96}, b_out, b_status{1};
    hipEvent_t ev[2] = {nullptr, nullptr};
    float ms = 0, ms_link = 0;             // the kernel of the last cg_hq_batch or permute call; k_hq_link of the last proving call
    ~HqState() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
};
void hq_state_free(void* s) { delete (HqState*)s; }

// under the handle's lock, after hipSetDevice
HqState& hq_state(PvkLinkView& v) {
    if (!*v.hq_state) {
        std::unique_ptr<HqState> fresh(new HqState());
        for (hipEvent_t& x : fresh->ev) CG_HIP(hipEventCreate(&x));
        *v.hq_state_free = hq_state_free;
        *v.hq_state = fresh.release();
    }
    HqState& h = *(HqState*)*v.hq_state;
    if (!h.uploads) {
        grow(h.consts, (uint64_t)POS_N_CONSTS);
        h2d_sync(h.consts.p, pos_consts().c, sizeof(F256) * POS_N_CONSTS, v.st);
        h.uploads = 1;
    }
    return h;
}

// cg_poseidon_p256_permute_batch (out_row 96) and cg_hq_batch (out_row 32): rows of 96 bytes in, in chunks
int hq_rows(cg_pvk* k, const uint8_t* in, uint64_t n, uint8_t* out, uint8_t* status, uint64_t out_row) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return CG_OK;
    if (!in || !out || !status) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    PvkLinkView v;
    pvk_link_handle(k, v);
    try {
        std::lock_guard<std::mutex> lk(*v.mu);
        CG_HIP(hipSetDevice(v.device));
        HqState& h = hq_state(v);
        const uint64_t chunk = n < DLMCHUNK ? n : DLMCHUNK;
        h.b_in.reserve(chunk);
        h.b_out.reserve(chunk, out_row);
        h.b_status.reserve(chunk);
        h.ms = 0;
        for (uint64_t off = 0; off < n; off += chunk) {
            const uint64_t m = n - off < chunk ? n - off : chunk;
            h.b_in.up(v.st, in, off, m);
            CG_HIP(hipEventRecord(h.ev[0], v.st));
            if (out_row == 96) k_hq_permute<<<ceil_div(m, DLMBLOCK), DLMBLOCK, 0, v.st>>>(h.consts.p, h.b_in.words(), m, h.b_out.words_mut(), h.b_status.bytes());
            else k_hq_hash<<<ceil_div(m, DLMBLOCK), DLMBLOCK, 0, v.st>>>(h.consts.p, h.b_in.words(), m, h.b_out.words_mut(), h.b_status.bytes());
            CG_KERNEL_CHECK();
            CG_HIP(hipEventRecord(h.ev[1], v.st));
            h.b_out.down(v.st, out, off, m);
            h.b_status.down(v.st, status, off, m);
            CG_HIP(hipStreamSynchronize(v.st));
            float t = 0;
            CG_HIP(hipEventElapsedTime(&t, h.ev[0], h.ev[1]));
            h.ms += t;
        }
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}

}  // namespace

namespace {
// cg_device_link_prove_batch (h_q_out null: h_Q is the caller's, h_len bytes per row) and cg_device_link_prove_hq_batch
// (h_q null, h_len 32: k_hq_link fills the chunk's rows on the device, and they come down into h_q_out)
int dlm_prove(cg_pvk* k, const uint8_t* io_types, uint64_t n_io, uint32_t pos0, uint32_t pos1, const uint8_t* committed, const uint8_t* openings,
              const uint8_t* rand, const uint8_t* h_q, uint32_t h_len, uint64_t n, const cg_device_link_made* out, uint8_t* e_out, uint8_t* status,
              uint8_t* h_q_out, bool on_device) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    PvkLinkView v;
    if (int rc = pvk_link_view(k, io_types, n_io, pos0, pos1, v)) return rc;
    if (h_len > DL_H_MAX) return fail(CG_ERR_INVALID_ARGUMENT, "h_len = %u: h_Q has at most %u bytes here", h_len, DL_H_MAX);
    if (n == 0) return CG_OK;
    if (!committed || !openings || !rand || (!on_device && h_len && !h_q) || (on_device && !h_q_out) || !out || !e_out || !status || !out->com1 ||
        !out->comz || !out->m || !out->pi0_c || !out->pi0_s || !out->pi1_c || !out->pi1_s)
        return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    try {
        std::lock_guard<std::mutex> lk(*v.mu);
        CG_HIP(hipSetDevice(v.device));
        if (!*v.make_state) {
            std::unique_ptr<DlmState> fresh(new DlmState());
            for (hipEvent_t& x : fresh->ev) CG_HIP(hipEventCreate(&x));
            *v.make_state_free = dlm_state_free;
            *v.make_state = fresh.release();
        }
        DlmState& s = *(DlmState*)*v.make_state;
        HqState* hq = on_device ? &hq_state(v) : nullptr;
        if (hq) hq->ms_link = 0;
        const uint64_t chunk = n < DLMCHUNK ? n : DLMCHUNK;
        s.b_comm.reserve(chunk, 64ull * v.n_com);
        s.b_hq.reserve(chunk, h_len);
        for (RowBuf* b : {&s.b_open, &s.b_rand, &s.b_com1, &s.b_comz, &s.b_m, &s.b_c0, &s.b_s0, &s.b_c1, &s.b_s1, &s.b_e, &s.b_status, &s.b_flags,
                          &s.b_opened, &s.b_pts, &s.b_r})
            b->reserve(chunk);
        grow(s.b_part, chunk * (uint64_t)DLM_N_TERMS);
        uint8_t consts[DL_CONSTS_LEN];     // the contexts and the compressed bases of this call's pos0 and pos1
        dl_link_consts(v.base_bytes, v.n_io, pos0, pos1, consts);
        grow(s.consts, sizeof(consts));
        h2d_sync(s.consts.p, consts, sizeof(consts), v.st);
        const uint64_t tab_stride = (uint64_t)FB_NWIN * FB_WIN;
        const G1Affine *tab_g = v.tab + pos0 * tab_stride, *tab_gp = v.tab + pos1 * tab_stride, *tab_h = v.tab + v.n_io * tab_stride;
        for (float& x : s.ms) x = 0;
        for (uint64_t off = 0; off < n; off += chunk) {
            const uint64_t m = n - off < chunk ? n - off : chunk;
            s.b_comm.up(v.st, committed, off, m);
            s.b_open.up(v.st, openings, off, m);
            s.b_rand.up(v.st, rand, off, m);
            if (!hq) s.b_hq.up(v.st, h_q, off, m);
            const DlmArgs a{s.b_comm.words(), v.n_com, v.ci0, v.ci1, s.b_open.words(), s.b_rand.words(), s.b_hq.bytes(), h_len, m};
            const DlmOut o{s.b_com1.words_mut(), s.b_comz.words_mut(), s.b_m.words_mut(), s.b_c0.words_mut(), s.b_s0.words_mut(),
                           s.b_c1.words_mut(), s.b_s1.words_mut(), s.b_e.words_mut(), s.b_status.bytes()};
            const uint32_t grid = ceil_div(m, DLMBLOCK);
            if (hq) {
                CG_HIP(hipEventRecord(hq->ev[0], v.st));
                k_hq_link<<<grid, DLMBLOCK, 0, v.st>>>(hq->consts.p, a, s.b_hq.words_mut());
                CG_KERNEL_CHECK();
            }
            CG_HIP(hipEventRecord(s.ev[0], v.st));
            k_dlm_check<<<grid, DLMBLOCK, 0, v.st>>>(a, s.b_flags.bytes());
            CG_KERNEL_CHECK();
            CG_HIP(hipEventRecord(s.ev[1], v.st));
            k_dlm_terms<<<ceil_div(m * DLM_N_TERMS, DLMBLOCK), DLMBLOCK, 0, v.st>>>(a, s.b_flags.bytes(), tab_g, tab_gp, tab_h, s.b_part.p);
            CG_KERNEL_CHECK();
            CG_HIP(hipEventRecord(s.ev[2], v.st));
            k_dlm_sum<<<ceil_div(m * DLM_N_OUT, DLMBLOCK), DLMBLOCK, 0, v.st>>>(a, s.b_flags.bytes(), s.b_part.p, o.com1, o.comz,
                                                                                s.b_pts.words_mut(), s.b_opened.bytes());
            CG_KERNEL_CHECK();
            CG_HIP(hipEventRecord(s.ev[3], v.st));
            k_dlm_pi0<<<grid, DLMBLOCK, 0, v.st>>>(a, s.b_flags.bytes(), s.b_opened.bytes(), s.consts.p, s.b_pts.words_mut(), o, s.b_r.words_mut());
            CG_KERNEL_CHECK();
            CG_HIP(hipEventRecord(s.ev[4], v.st));
            k_dlm_lhs1<<<grid, DLMBLOCK, 0, v.st>>>(m, s.b_status.bytes(), s.b_r.words(), tab_h, s.b_pts.words_mut());
            CG_KERNEL_CHECK();
            CG_HIP(hipEventRecord(s.ev[5], v.st));
            k_dlm_pi1<<<grid, DLMBLOCK, 0, v.st>>>(a, s.consts.p, s.b_pts.words(), s.b_r.words(), o);
            CG_KERNEL_CHECK();
            CG_HIP(hipEventRecord(s.ev[6], v.st));
            s.b_com1.down(v.st, out->com1, off, m);
            s.b_comz.down(v.st, out->comz, off, m);
            s.b_m.down(v.st, out->m, off, m);
            s.b_c0.down(v.st, out->pi0_c, off, m);
            s.b_s0.down(v.st, out->pi0_s, off, m);
            s.b_c1.down(v.st, out->pi1_c, off, m);
            s.b_s1.down(v.st, out->pi1_s, off, m);
            s.b_e.down(v.st, e_out, off, m);
            s.b_status.down(v.st, status, off, m);
            if (hq) s.b_hq.down(v.st, h_q_out, off, m);
            CG_HIP(hipStreamSynchronize(v.st));
            for (int i = 0; i < 6; ++i) {
                float t = 0;
                CG_HIP(hipEventElapsedTime(&t, s.ev[i], s.ev[i + 1]));
                s.ms[i] += t;
            }
            if (hq) {
                float t = 0;
                CG_HIP(hipEventElapsedTime(&t, hq->ev[0], s.ev[0]));
                hq->ms_link += t;
                // a row that a later stage found malformed (an opening that does not open) has every output zero, h_Q included
                for (uint64_t p = off; p < off + m; ++p)
                    if (status[p] != CG_SHOW_MADE) memset(h_q_out + 32 * p, 0, 32);
            }
        }
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}
}  // namespace

extern "C" int cg_device_link_prove_batch(cg_pvk* k, const uint8_t* io_types, uint64_t n_io, uint32_t pos0, uint32_t pos1,
                                          const uint8_t* committed, const uint8_t* openings, const uint8_t* rand, const uint8_t* h_q,
                                          uint32_t h_len, uint64_t n, const cg_device_link_made* out, uint8_t* e_out, uint8_t* status) {
    return dlm_prove(k, io_types, n_io, pos0, pos1, committed, openings, rand, h_q, h_len, n, out, e_out, status, nullptr, false);
}

// the same with h_Q computed on the device from q0, q1 (openings) and z (rand[0]); its 32 bytes per row come back in h_q_out
extern "C" int cg_device_link_prove_hq_batch(cg_pvk* k, const uint8_t* io_types, uint64_t n_io, uint32_t pos0, uint32_t pos1,
                                             const uint8_t* committed, const uint8_t* openings, const uint8_t* rand, uint64_t n,
                                             const cg_device_link_made* out, uint8_t* e_out, uint8_t* status, uint8_t* h_q_out) {
    return dlm_prove(k, io_types, n_io, pos0, pos1, committed, openings, rand, nullptr, 32, n, out, e_out, status, h_q_out, true);
}

// Poseidon over P-256's base field, width 3: n states of three canonical elements (32 bytes little-endian each) -> the
// permuted states.  A row with an element >= p is CG_SHOW_MALFORMED, that row alone, and its output zero.
extern "C" int cg_poseidon_p256_permute_batch(cg_pvk* k, const uint8_t* states, uint64_t n, uint8_t* out, uint8_t* status) {
    return hq_rows(k, states, n, out, status, 96);
}

// h_Q = compute_hQ(q0, q1, z) for n rows of three canonical Fr -> 32 bytes big-endian per row, as cg_device_link_rows.h_q
// takes them with h_len = 32.  A row with a scalar >= r is CG_SHOW_MALFORMED, that row alone, and its output zero.
extern "C" int cg_hq_batch(cg_pvk* k, const uint8_t* q, uint64_t n, uint8_t* h_q_out, uint8_t* status) {
    return hq_rows(k, q, n, h_q_out, status, 32);
}

// Diagnostic: ms[0] the kernel of the handle's last cg_hq_batch or cg_poseidon_p256_permute_batch, ms[1] k_hq_link of its
// last cg_device_link_prove_hq_batch, by HIP events, summed over the chunks; *uploads how often the Poseidon constants went
// up to this handle (0 before the first call that needs them, 1 ever after)
extern "C" int cg_hq_last_kernel_ms(cg_pvk* k, float ms[2], uint32_t* uploads) {
    if (!k || !ms || !uploads) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    PvkLinkView v;
    pvk_link_handle(k, v);
    std::lock_guard<std::mutex> lk(*v.mu);
    const HqState* h = (const HqState*)*v.hq_state;
    ms[0] = h ? h->ms : 0.f;
    ms[1] = h ? h->ms_link : 0.f;
    *uploads = h ? h->uploads : 0u;
    return CG_OK;
}

// Diagnostic: what the six kernels of the handle's last cg_device_link_prove_batch took, by HIP events, summed over its
// chunks: k_dlm_check, k_dlm_terms, k_dlm_sum, k_dlm_pi0, k_dlm_lhs1, k_dlm_pi1
extern "C" int cg_device_link_prove_last_kernel_ms(cg_pvk* k, float ms[6]) {
    if (!k || !ms) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    PvkLinkView v;
    pvk_link_handle(k, v);
    std::lock_guard<std::mutex> lk(*v.mu);
    const DlmState* s = (const DlmState*)*v.make_state;
    for (int i = 0; i < 6; ++i) ms[i] = s ? s->ms[i] : 0.f;
    return CG_OK;
}
