// The BN254 half of a device proof on the GPU: `DeviceProof::verify` (creds/src/device.rs:168-213) short of pi2, the Spartan
// proof over T-256, for a batch of device-bound showings under one cg_pvk.  What `verify_show` / `verify_show_mdl` run per
// showing after `ShowGroth16::verify` (creds/src/lib.rs:660-680, :893-913).
//
// With g = gamma_abc_g1[pos0 + 1], g' = gamma_abc_g1[pos1 + 1], h = delta_g1, com0 and com1_orig the showing's own committed
// points of pos0 and pos1, and (e1, e2) the SHA-256 challenge over the commitments' text forms (device_link.hpp):
//   pi0 (eq_pos (0, 0))   k_0 = s00 g' + s01 h + c0 com1_orig         k_1 = s10 g + s11 h + c0 com1
//   the recombination     lhs1 = com0 + e1 com1 + e2 comz - m g
//   pi1                   k_0 = t0 h + c1 lhs1                        k_1 = u0 g + u1 h + c1 comz
// c1 lhs1 is taken as FOUR chains with merged scalars beside all the others - c1 com0 + (c1 e1) com1 + (c1 e2) comz - (c1 m) g,
// the last one a walk through g's table - not as one chain behind the sum of lhs1: the chip is far from full at any batch
// size this call sees, so two more lanes per proof cost less than a second chain's length on every proof's critical path
// (profiles/device_link.md).  A chunk of proofs runs four kernels on the key's own non-blocking stream, under its lock, with
// nothing coming down in between; scalars and partials are laid out TERM-MAJOR within the chunk (term t of proof p at
// t·m + p), so that a wave holds one kind of term, as k_rv_terms has it:
//   k_dl_check      one lane per proof: ark's checked deserialisation of com0, com1_orig, com1 and comz; the digest of the
//                   message (sha256.hpp, the block and one coordinate's digits in LDS) -> e_out; the scalar stage
//                   (device_link.hpp: range checks, eq_pos, the three merged scalars)                     -> one flag byte
//   k_dl_terms      one lane per (term, proof): nine walks through the key's tables of g, g' and h; then, in workgroups of
//                   their own, the eight variable-base chains, the two 128-bit ones last                  -> XYZZ partials
//   k_dl_sum        one lane per (output point, proof): lhs1 and the four k, by the general `add` throughout - chosen proofs
//                   make partials coincide or cancel -, normalised, as ark-serialize's compressed bytes
//   k_dl_challenge  one lane per proof: both DLogPoK transcripts (merlin.hpp's ml_dlog_shape_challenge, the sponge in LDS)
//                   over the compressed bases, the k and the y as their bytes stand; c' == c, eq_pos     -> the verdicts
// A malformed proof costs nothing after k_dl_check: every later lane of it returns at once.
// k_dl_check and k_dl_challenge do arithmetic on bytes and words only and declare no private segment.
#include <memory>

#include "common.hpp"
#include "device_link.hpp"
#include "fixed_base.hpp"
#include "host_parallel.hpp"
#include "key_handle.hpp"

using namespace cg;

namespace {

constexpr uint64_t DLCHUNK = 1u << 15;     // proofs per launch set; 3 KB of device memory per proof
constexpr int DLBLOCK = 64;
constexpr int DL_LANE_LDS = SHA_BLOCK + DL_DIGITS_ROOM;      // 148 bytes = 37 words per lane: an odd stride, no bank shared

// one chunk's arrays on the device, as the caller laid them out
struct DlArgs {
    const uint32_t* committed;             // n_com x 16 words per proof; com0 at ci0, com1_orig at ci1
    uint32_t n_com, ci0, ci1;
    const uint32_t *com1, *comz;           // 16 words per proof
    const uint8_t* h_q;                    // h_len bytes per proof
    uint32_t h_len;
    const uint32_t *m, *pi0_c, *pi0_s, *pi1_c, *pi1_s;      // 8, 8, 32, 8, 24
    uint64_t n;
    __device__ const uint32_t* com0(uint64_t p) const { return committed + 16 * (p * n_com + ci0); }
    __device__ const uint32_t* com1_orig(uint64_t p) const { return committed + 16 * (p * n_com + ci1); }
};

__global__ __launch_bounds__(DLBLOCK) void k_dl_check(DlArgs a, uint32_t* __restrict__ e_out, uint32_t* __restrict__ scal,
                                                     uint8_t* __restrict__ flags) {
    __shared__ __attribute__((aligned(4))) uint8_t lds[DLBLOCK * DL_LANE_LDS];
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    uint8_t* mine = lds + DL_LANE_LDS * threadIdx.x;
    uint32_t* e = e_out + 8 * p;
    dl_challenge_digest(mine, mine + SHA_BLOCK, a.pi0_c + 8 * p, a.com0(p), a.com1 + 16 * p, a.comz + 16 * p, a.h_q + p * a.h_len, a.h_len,
                        (uint8_t*)e);
    const DlIn in{a.m + 8 * p, a.pi0_c + 8 * p, a.pi0_s + 32 * p, a.pi1_c + 8 * p, a.pi1_s + 24 * p, e};
    uint32_t f = dl_scalars(in, scal + 8 * p, a.n);
    bool ok = true;
    (void)dev_g1(a.com0(p), ok);
    (void)dev_g1(a.com1_orig(p), ok);
    (void)dev_g1(a.com1 + 16 * p, ok);
    (void)dev_g1(a.comz + 16 * p, ok);
    if (!ok) f = DL_MALFORMED;
    if (f & DL_MALFORMED)
        for (int l = 0; l < 8; ++l) e[l] = 0;
    flags[p] = (uint8_t)f;
}

__global__ __launch_bounds__(DLBLOCK) void k_dl_terms(DlArgs a, const uint32_t* __restrict__ e, const uint32_t* __restrict__ scal,
                                                     const uint8_t* __restrict__ flags, const G1Affine* __restrict__ tab_g,
                                                     const G1Affine* __restrict__ tab_gp, const G1Affine* __restrict__ tab_h,
                                                     G1XYZZ* __restrict__ part) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t m = a.n, n_fixed_lanes = m * DL_N_FIXED;
    if (g < n_fixed_lanes) {
        const uint32_t t = (uint32_t)(g / m);
        const uint64_t p = g % m;
        if (flags[p] & DL_MALFORMED) return;
        const uint32_t* x;
        const G1Affine* tb;
        switch (t) {
            case DL_F_S00: x = a.pi0_s + 32 * p; tb = tab_gp; break;
            case DL_F_S01: x = a.pi0_s + 32 * p + 8; tb = tab_h; break;
            case DL_F_S10: x = a.pi0_s + 32 * p + 16; tb = tab_g; break;
            case DL_F_S11: x = a.pi0_s + 32 * p + 24; tb = tab_h; break;
            case DL_F_T0: x = a.pi1_s + 24 * p; tb = tab_h; break;
            case DL_F_U0: x = a.pi1_s + 24 * p + 8; tb = tab_g; break;
            case DL_F_U1: x = a.pi1_s + 24 * p + 16; tb = tab_h; break;
            case DL_F_M: x = a.m + 8 * p; tb = tab_g; break;
            default: x = scal + 8 * (DL_S_C1M * m + p); tb = tab_g; break;
        }
        part[g] = fixed_base_mul(tb, x);
        return;
    }
    // the variable-base lanes (chains several times as long) start at a workgroup of their own
    const uint64_t var_at = (n_fixed_lanes + DLBLOCK - 1) / DLBLOCK * DLBLOCK;
    if (g < var_at || g - var_at >= m * DL_N_VAR) return;
    const uint64_t v = g - var_at;
    const uint32_t t = (uint32_t)(v / m);
    const uint64_t p = v % m;
    if (flags[p] & DL_MALFORMED) return;
    const uint32_t *pt, *k;
    int bits = 254;                                               // a challenge has 248 bits, but a forged c is any scalar below r
    switch (t) {
        case DL_V_C0_COM1O: pt = a.com1_orig(p); k = a.pi0_c + 8 * p; break;
        case DL_V_C0_COM1: pt = a.com1 + 16 * p; k = a.pi0_c + 8 * p; break;
        case DL_V_C1_COMZ: pt = a.comz + 16 * p; k = a.pi1_c + 8 * p; break;
        case DL_V_C1_COM0: pt = a.com0(p); k = a.pi1_c + 8 * p; break;
        case DL_V_C1E1_COM1: pt = a.com1 + 16 * p; k = scal + 8 * (DL_S_C1E1 * m + p); break;
        case DL_V_C1E2_COMZ: pt = a.comz + 16 * p; k = scal + 8 * (DL_S_C1E2 * m + p); break;
        case DL_V_E1_COM1: pt = a.com1 + 16 * p; k = e + 8 * p; bits = 128; break;
        default: pt = a.comz + 16 * p; k = e + 8 * p + 4; bits = 128; break;
    }
    part[(DL_N_FIXED + t) * m + p] = scalar_mul_mixed(dev_g1_unchecked(pt), k, bits);
}

// the terms of output point o, one byte each from the lowest: a fixed-base term t as t, a variable-base one as
// DL_N_FIXED + t, with DL_SUBTRACT where the term is subtracted; DL_NO_TERM ends the list
constexpr uint64_t DL_SUBTRACT = 0x80, DL_NO_TERM = 0xff;
constexpr uint64_t dl_list(uint64_t t0, uint64_t t1, uint64_t t2, uint64_t t3 = DL_NO_TERM, uint64_t t4 = DL_NO_TERM) {
    return t0 | t1 << 8 | t2 << 16 | t3 << 24 | t4 << 32 | DL_NO_TERM << 40;
}
constexpr uint64_t dl_var(uint64_t t) { return DL_N_FIXED + t; }

__global__ __launch_bounds__(DLBLOCK) void k_dl_sum(DlArgs a, const uint8_t* __restrict__ flags, const G1XYZZ* __restrict__ part,
                                                   uint32_t* __restrict__ pts) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t m = a.n;
    if (g >= m * DL_N_OUT) return;
    const uint32_t o = (uint32_t)(g / m);
    const uint64_t p = g % m;
    uint32_t* out = pts + 8 * (DL_N_OUT * p + o);
    if (flags[p] & DL_MALFORMED) {
        for (int l = 0; l < 8; ++l) out[l] = 0;
        return;
    }
    const uint64_t list = o == DL_O_LHS1  ? dl_list(dl_var(DL_V_E1_COM1), dl_var(DL_V_E2_COMZ), DL_F_M | DL_SUBTRACT)
                          : o == DL_O_K00 ? dl_list(DL_F_S00, DL_F_S01, dl_var(DL_V_C0_COM1O))
                          : o == DL_O_K01 ? dl_list(DL_F_S10, DL_F_S11, dl_var(DL_V_C0_COM1))
                          : o == DL_O_K10 ? dl_list(dl_var(DL_V_C1_COM0), dl_var(DL_V_C1E1_COM1), dl_var(DL_V_C1E2_COMZ), DL_F_C1M | DL_SUBTRACT, DL_F_T0)
                                          : dl_list(DL_F_U0, DL_F_U1, dl_var(DL_V_C1_COMZ));
    G1XYZZ acc = G1XYZZ::inf();
    if (o == DL_O_LHS1) acc = G1XYZZ::from_affine(dev_g1_unchecked(a.com0(p)));
#pragma nounroll
    for (int j = 0; j < 6; ++j) {
        const uint32_t t = (uint32_t)(list >> (8 * j)) & 0xffu;
        if (t == DL_NO_TERM) break;
        const G1XYZZ q = part[(uint64_t)(t & 0x7fu) * m + p];
        add(acc, (t & DL_SUBTRACT) ? neg(q) : q);
    }
    dev_put_g1(to_affine(acc), out, true);
}

// consts: the two contexts (2 x DL_CTX_LEN bytes), then the bases g', h, g, h compressed (4 x 32): pi0 absorbs all four,
// pi1 the last three.  y_cmp: per proof com1_orig, com1, lhs1 and comz compressed; c_prime: per proof the two challenges.
__global__ __launch_bounds__(DLBLOCK) void k_dl_challenge(DlArgs a, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ pts,
                                                         const uint8_t* __restrict__ consts, uint32_t* __restrict__ y_cmp,
                                                         uint32_t* __restrict__ c_prime, uint8_t* __restrict__ verdict,
                                                         uint8_t* __restrict__ parts) {
    __shared__ __attribute__((aligned(8))) uint8_t sponge[DLBLOCK * ML_STATE];
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    if (flags[p] & DL_MALFORMED) {
        verdict[p] = parts[2 * p] = parts[2 * p + 1] = CG_VERIFY_MALFORMED;
        return;
    }
    uint32_t* y = y_cmp + 32 * p;
    ml_compress_g1(a.com1_orig(p), y);
    ml_compress_g1(a.com1 + 16 * p, y + 8);
    for (int l = 0; l < 8; ++l) y[16 + l] = pts[8 * (DL_N_OUT * p + DL_O_LHS1) + l];
    ml_compress_g1(a.comz + 16 * p, y + 24);
    uint32_t same = 0;                                            // bit t: transcript t gives the challenge the proof states
#pragma nounroll
    for (uint32_t t = 0; t < 2; ++t) {
        uint32_t* c = c_prime + 8 * (2 * p + t);
        ml_dlog_shape_challenge(sponge + ML_STATE * threadIdx.x, consts + DL_CTX_LEN * t, DL_CTX_LEN, 2u,
                                [=](uint32_t i) { return t == 1 && i == 0 ? 1u : 2u; }, consts + 2 * DL_CTX_LEN + 32 * t,
                                (const uint8_t*)(pts + 8 * (DL_N_OUT * p + DL_O_K00 + 2 * t)), (const uint8_t*)(y + 16 * t), (uint8_t*)c);
        const uint32_t* given = (t ? a.pi1_c : a.pi0_c) + 8 * p;
        uint32_t differ = 0;
        for (int l = 0; l < 8; ++l) differ |= c[l] ^ given[l];
        same |= (differ == 0 ? 1u : 0u) << t;
    }
    const bool ok0 = (same & 1u) && (flags[p] & DL_EQ_POS), ok1 = (same & 2u) != 0;
    parts[2 * p] = ok0 ? CG_VERIFY_ACCEPT : CG_VERIFY_REJECT;
    parts[2 * p + 1] = ok1 ? CG_VERIFY_ACCEPT : CG_VERIFY_REJECT;
    verdict[p] = ok0 && ok1 ? CG_VERIFY_ACCEPT : CG_VERIFY_REJECT;
}

// The per-call arrays of a key's device link: grown to the largest chunk seen, never shrunk; bytes are the caller's.
struct DlState {
    RowBuf b_comm, b_com1{64}, b_comz{64}, b_hq, b_m{32}, b_c0{32}, b_s0{128}, b_c1{32}, b_s1{96};
    RowBuf b_e{32}, b_pts{32 * DL_N_OUT}, b_y{128}, b_cprime{64}, b_flags{1}, b_verdict{1}, b_parts{2};
    DevBuf<uint32_t> b_scal;               // DL_N_SCALARS per proof, term-major
    DevBuf<G1XYZZ> b_part;                 // one partial per (term, proof)
    DevBuf<uint8_t> consts;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};      // around the four kernels of a chunk
    float ms[4] = {0, 0, 0, 0};                                            // of the last call, summed over its chunks
    ~DlState() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
};
void dl_state_free(void* s) { delete (DlState*)s; }

}  // namespace

extern "C" int cg_device_link_verify_batch(cg_pvk* k, const uint8_t* io_types, uint64_t n_io, uint32_t pos0, uint32_t pos1,
                                           const uint8_t* committed, const cg_device_link_rows* rows, uint32_t h_len, uint64_t n,
                                           uint8_t* verdicts, uint8_t* part_verdicts, uint8_t* e_out) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    PvkLinkView v;
    if (int rc = pvk_link_view(k, io_types, n_io, pos0, pos1, v)) return rc;
    if (h_len > DL_H_MAX) return fail(CG_ERR_INVALID_ARGUMENT, "h_len = %u: h_Q has at most %u bytes here", h_len, DL_H_MAX);
    if (n == 0) return CG_OK;
    if (!committed || !rows || !verdicts || !e_out || !rows->com1 || !rows->comz || (h_len && !rows->h_q) || !rows->m || !rows->pi0_c ||
        !rows->pi0_s || !rows->pi1_c || !rows->pi1_s)
        return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    try {
        std::lock_guard<std::mutex> lk(*v.mu);
        CG_HIP(hipSetDevice(v.device));
        if (!*v.state) {
            std::unique_ptr<DlState> fresh(new DlState());
            for (hipEvent_t& x : fresh->ev) CG_HIP(hipEventCreate(&x));
            *v.state_free = dl_state_free;
            *v.state = fresh.release();
        }
        DlState& s = *(DlState*)*v.state;
        const uint64_t chunk = n < DLCHUNK ? n : DLCHUNK;
        s.b_comm.reserve(chunk, 64ull * v.n_com);
        s.b_hq.reserve(chunk, h_len);
        for (RowBuf* b : {&s.b_com1, &s.b_comz, &s.b_m, &s.b_c0, &s.b_s0, &s.b_c1, &s.b_s1, &s.b_e, &s.b_pts, &s.b_y, &s.b_cprime, &s.b_flags,
                          &s.b_verdict, &s.b_parts})
            b->reserve(chunk);
        grow(s.b_scal, chunk * 8 * DL_N_SCALARS);
        grow(s.b_part, chunk * (uint64_t)(DL_N_FIXED + DL_N_VAR));
        // the contexts and the compressed bases of this call's pos0 and pos1
        uint8_t consts[DL_CONSTS_LEN];
        dl_link_consts(v.base_bytes, v.n_io, pos0, pos1, consts);
        grow(s.consts, sizeof(consts));
        h2d_sync(s.consts.p, consts, sizeof(consts), v.st);
        const uint64_t tab_stride = (uint64_t)FB_NWIN * FB_WIN;
        const G1Affine *tab_g = v.tab + pos0 * tab_stride, *tab_gp = v.tab + pos1 * tab_stride, *tab_h = v.tab + v.n_io * tab_stride;
        for (float& x : s.ms) x = 0;
        for (uint64_t off = 0; off < n; off += chunk) {
            const uint64_t m = n - off < chunk ? n - off : chunk;
            s.b_comm.up(v.st, committed, off, m);
            s.b_com1.up(v.st, rows->com1, off, m);
            s.b_comz.up(v.st, rows->comz, off, m);
            s.b_hq.up(v.st, rows->h_q, off, m);
            s.b_m.up(v.st, rows->m, off, m);
            s.b_c0.up(v.st, rows->pi0_c, off, m);
            s.b_s0.up(v.st, rows->pi0_s, off, m);
            s.b_c1.up(v.st, rows->pi1_c, off, m);
            s.b_s1.up(v.st, rows->pi1_s, off, m);
            const DlArgs a{s.b_comm.words(), v.n_com, v.ci0, v.ci1, s.b_com1.words(), s.b_comz.words(), s.b_hq.bytes(), h_len, s.b_m.words(),
                           s.b_c0.words(), s.b_s0.words(), s.b_c1.words(), s.b_s1.words(), m};
            const uint32_t grid = ceil_div(m, DLBLOCK);
            CG_HIP(hipEventRecord(s.ev[0], v.st));
            k_dl_check<<<grid, DLBLOCK, 0, v.st>>>(a, s.b_e.words_mut(), s.b_scal.p, s.b_flags.bytes());
            CG_KERNEL_CHECK();
            CG_HIP(hipEventRecord(s.ev[1], v.st));
            k_dl_terms<<<ceil_div(m * DL_N_FIXED, DLBLOCK) + ceil_div(m * DL_N_VAR, DLBLOCK), DLBLOCK, 0, v.st>>>(
                a, s.b_e.words(), s.b_scal.p, s.b_flags.bytes(), tab_g, tab_gp, tab_h, s.b_part.p);
            CG_KERNEL_CHECK();
            CG_HIP(hipEventRecord(s.ev[2], v.st));
            k_dl_sum<<<ceil_div(m * DL_N_OUT, DLBLOCK), DLBLOCK, 0, v.st>>>(a, s.b_flags.bytes(), s.b_part.p, s.b_pts.words_mut());
            CG_KERNEL_CHECK();
            CG_HIP(hipEventRecord(s.ev[3], v.st));
            k_dl_challenge<<<grid, DLBLOCK, 0, v.st>>>(a, s.b_flags.bytes(), s.b_pts.words(), s.consts.p, s.b_y.words_mut(),
                                                       s.b_cprime.words_mut(), s.b_verdict.bytes(), s.b_parts.bytes());
            CG_KERNEL_CHECK();
            CG_HIP(hipEventRecord(s.ev[4], v.st));
            s.b_verdict.down(v.st, verdicts, off, m);
            s.b_parts.down(v.st, part_verdicts, off, m);
            s.b_e.down(v.st, e_out, off, m);
            CG_HIP(hipStreamSynchronize(v.st));
            for (int i = 0; i < 4; ++i) {
                float t = 0;
                CG_HIP(hipEventElapsedTime(&t, s.ev[i], s.ev[i + 1]));
                s.ms[i] += t;
            }
        }
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}

// Diagnostic: what the four kernels of the handle's last cg_device_link_verify_batch took, by HIP events, summed over its
// chunks: k_dl_check, k_dl_terms, k_dl_sum, k_dl_challenge
extern "C" int cg_device_link_last_kernel_ms(cg_pvk* k, float ms[4]) {
    if (!k || !ms) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    PvkLinkView v;
    pvk_link_handle(k, v);
    std::lock_guard<std::mutex> lk(*v.mu);
    const DlState* s = (const DlState*)*v.state;
    for (int i = 0; i < 4; ++i) ms[i] = s ? s->ms[i] : 0.f;
    return CG_OK;
}

// ---- cg_revealed_digest_batch: the host instance of sha256.hpp -----------------------------------------------------------
// lib.rs:590-603 per hashed attribute: SHA-256 of the preimage, its first 31 bytes through `bits_to_num` (utils.rs:78-94):
// byte j of the little-endian result is digest byte j with its bits mirrored, and byte 31 is zero.
extern "C" int cg_revealed_digest_batch(const uint8_t* data, const uint64_t* offsets, uint64_t n_items, uint8_t* out) {
    if (n_items == 0) return CG_OK;
    if (!offsets || !out) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    for (uint64_t i = 0; i < n_items; ++i) {
        if (offsets[i + 1] < offsets[i]) return fail(CG_ERR_INVALID_ARGUMENT, "offsets[%llu] is above offsets[%llu]", (unsigned long long)i, (unsigned long long)(i + 1));
        if (offsets[i + 1] - offsets[i] > 0xffffffffull)
            return fail(CG_ERR_INVALID_ARGUMENT, "item %llu is longer than 2^32 - 1 bytes", (unsigned long long)i);
    }
    if (offsets[n_items] > offsets[0] && !data) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    try {
        parallel_ranges(n_items, 64, [&](uint64_t lo, uint64_t hi) {
            alignas(8) uint8_t blk[SHA_BLOCK];
            uint8_t d[32];
            for (uint64_t i = lo; i < hi; ++i) {
                sha256_of(blk, data + offsets[i], offsets[i + 1] - offsets[i], d);
                uint8_t* o = out + 32 * i;
                for (int j = 0; j < 31; ++j) {
                    uint8_t b = d[j], r = 0;
                    for (int t = 0; t < 8; ++t) r |= (uint8_t)(((b >> t) & 1u) << (7 - t));
                    o[j] = r;
                }
                o[31] = 0;
            }
        });
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}
