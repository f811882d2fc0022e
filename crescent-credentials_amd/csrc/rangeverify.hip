// Verifying range proofs on the GPU: `ShowRange::verify` -> `RangeProof::verify_n_bits` (creds/src/rangeproof.rs:342-424)
// for a batch of proofs under one `RangeProofVK`, up to the Merlin transcripts, which stay with the host (c and rho come
// in, the DLEQ's recomputed commitments go out), and with the two randomizers of `KZG10::batch_check` given by the caller.
//
// A cg_range_vk holds, on a device, the 91 line coefficients of prepared h and of prepared beta_h, fixed-base tables
// (fixed_base.hpp) of g, gamma_g and the four com_f_basis points and, per registered slot, of one pair of Pedersen bases.
// cg_range_verify_batch runs five kernels per chunk of showings on the handle's own non-blocking stream.  Scalars and
// partials are laid out TERM-MAJOR within the chunk (term t of showing p at t·m + p), so that a wave holds one kind of term:
// one table for a fixed-base wave, one chain length for a variable-base wave.
//   k_rv_check    one lane per showing: the scalar stage (rangeverify.hpp: range checks, rho^n, one inversion, the identity
//                 and eq_pos bits, the ten merged term scalars) and ark's checked deserialisation of the seven points
//                                                                                                     -> one flag byte
//   k_rv_terms    one lane per (term, showing): the fixed-base terms (Σ r_i v_i)·g, (Σ r_i random_v_i)·gamma_g and, with a
//                 DLEQ, the six responses on the slot's bases and com_f_basis, from the tables; then, in workgroups of their
//                 own, the variable-base chains: eight of batch_check, c_dleq·ped_com and c_dleq·com_f.  A chain is as long
//                 as its scalar: 128 doublings for r_1·W_gw and r_2·W_w^, 129 for (1 + r_1)·com_g, 254 for the rest
//                                                                                                     -> XYZZ partials
//   k_rv_sum      one lane per (output point, showing): total_c, -total_w (affine, for the pairing), k_0 and k_1 (ark-serialize
//                 compressed, what the transcript absorbs under b"k").  The general `add` throughout: chosen proofs make
//                 partials coincide or cancel
//   k_rv_miller   one lane per showing: multi_miller_loop<0> over (-total_w, prepared beta_h), (total_c, prepared h); a pair
//                 whose G1 point is O, or whose key point is, is dropped as ark's multi_miller_loop drops it
//   k_rv_final    one lane per showing: final exponentiation, == one, and the two bits               -> one verdict byte
// A malformed showing costs nothing after k_rv_check: every later lane of it returns at once.
// cg_range_verify_proofs_batch is the same call with the transcripts on the device (merlin.hpp): k_rv_challenges in front
// derives c and rho, k_rv_challenge_dleq behind recomputes the DLEQ's challenge and compares it with pok_c.
// Both entries are run_range_verify over rv_chunk, one chunk's copies and kernels; rangeverify.hpp's internal entry hands the
// same rv_chunk to cg_verify_showings_batch (verify.hip) with ped_com and the verdicts as device pointers.
// The handle's device, stream and lock, the timing of the two stages, the slots and the per-call arrays are key_handle.hpp's
// (KeyHandle, StageTimer, PedersenSlots, RowBuf), shared with cg_pvk and cg_range_pk; the chains are scalar_mul_mixed.
#include <memory>

#include "common.hpp"
#include "fixed_base.hpp"
#include "key_handle.hpp"
#include "pairing.hpp"
#include "pairing_team.hpp"
#include "rangeverify.hpp"

using namespace cg;

namespace {

// showings per launch set.  A call is bound by latency, not by width: the pairing kernels hold one wave per SIMD, so the
// chip takes 65536 showings side by side and a chunk of 1 and one of 4096 take the same 46 ms (profiles/range_verify.md);
// chunks run one after the other, so a chunk is as large as cg_verify_batch's.  4 KB of device memory per showing.
constexpr uint64_t RVCHUNK = 1u << 15;
constexpr int RVBLOCK = 64;
constexpr int NC = PairingConsts::N_COEFFS;
constexpr uint32_t RV_VK_BYTES = 640;      // g | gamma_g | h | beta_h | com_f_basis[4]
// the key's tables: g, gamma_g, then com_f_basis
enum { TAB_G = 0, TAB_GAMMA_G = 1, TAB_CFB = 2, N_TABS = 6 };
constexpr uint32_t N_FIX_DLEQ = RP_N_RESP, N_VAR_DLEQ = 2;

// one call's arrays on the device, as the caller laid them out
struct RvArgs {
    const uint32_t *ped_com, *com_f, *com_g, *com_q;      // 16 words per showing
    const uint32_t *evals, *proofs;                       // 24, 72
    const uint32_t *c, *rho, *rz;                         // 8, 8, 8
    const uint32_t *pok_c, *pok_s;                        // 8, 48; null without a DLEQ
    uint64_t m;
    uint32_t n_fixed, n_var;                              // 2 + 6, 8 + 2 with a DLEQ
};

__global__ __launch_bounds__(RVBLOCK) void k_rv_check(RangeConsts kc, RvArgs a, uint32_t* __restrict__ scal, uint8_t* __restrict__ flags) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.m) return;
    const RvIn in{a.evals + 24 * p, a.proofs + 72 * p, a.c + 8 * p, a.rho + 8 * p, a.rz + 8 * p,
                  a.pok_c ? a.pok_c + 8 * p : nullptr, a.pok_c ? a.pok_s + 48 * p : nullptr};
    uint32_t f = rv_scalars(kc, in, scal + 8 * p, a.m);
    bool ok = true;
    (void)dev_g1(a.com_f + 16 * p, ok);
    (void)dev_g1(a.com_g + 16 * p, ok);
    (void)dev_g1(a.com_q + 16 * p, ok);
    for (int j = 0; j < 3; ++j) (void)dev_g1(a.proofs + 72 * p + 24 * j, ok);
    if (a.pok_c) (void)dev_g1(a.ped_com + 16 * p, ok);            // without a DLEQ the commitment is not read
    if (!ok) f = RV_MALFORMED;
    flags[p] = (uint8_t)f;
}

__global__ __launch_bounds__(RVBLOCK) void k_rv_terms(RvArgs a, const uint32_t* __restrict__ scal, const uint8_t* __restrict__ flags,
                                                     const G1Affine* __restrict__ tab, const G1Affine* __restrict__ tab_slot,
                                                     G1XYZZ* __restrict__ part) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t m = a.m, n_fixed_lanes = m * a.n_fixed;
    if (g < n_fixed_lanes) {
        const uint32_t t = (uint32_t)(g / m);
        const uint64_t p = g % m;
        if (flags[p] & RV_MALFORMED) return;
        const uint32_t* x;
        const G1Affine* tb;
        if (t < RV_N_FIX_KZG) {
            x = scal + 8 * ((RV_N_VAR_KZG + t) * m + p);
            tb = tab + (uint64_t)(TAB_G + t) * FB_NWIN * FB_WIN;
        } else {                                                  // s_00 s_01 on the slot's bases, s_10..s_13 on com_f_basis
            const uint32_t j = t - RV_N_FIX_KZG;
            x = a.pok_s + 8 * (RP_N_RESP * p + j);
            tb = j < 2 ? tab_slot + (uint64_t)j * FB_NWIN * FB_WIN : tab + (uint64_t)(TAB_CFB + j - 2) * FB_NWIN * FB_WIN;
        }
        part[g] = fixed_base_mul(tb, x);
        return;
    }
    // the variable-base lanes (chains several times as long) start at a workgroup of their own
    const uint64_t var_at = (n_fixed_lanes + RVBLOCK - 1) / RVBLOCK * RVBLOCK;
    if (g < var_at || g - var_at >= m * a.n_var) return;
    const uint64_t v = g - var_at;
    const uint32_t t = (uint32_t)(v / m);
    const uint64_t p = v % m;
    if (flags[p] & RV_MALFORMED) return;
    const uint32_t *pt, *k;
    int bits = 254;
    if (t < RV_N_VAR_KZG) {
        k = scal + 8 * (t * m + p);
        bits = rv_scalar_bits((int)t);
        pt = t == RV_COM_G ? a.com_g + 16 * p : t == RV_COM_F ? a.com_f + 16 * p : t == RV_COM_Q ? a.com_q + 16 * p
             : a.proofs + 72 * p + 24 * (t == RV_W_G ? 0 : (t == RV_W_GW || t == RV_TW_GW) ? 1 : 2);
    } else {                                                      // c_dleq·y_i: y = [ped_com, com_f]  (c < r < 2^254)
        k = a.pok_c + 8 * p;
        pt = t == RV_N_VAR_KZG ? a.ped_com + 16 * p : a.com_f + 16 * p;
    }
    part[(a.n_fixed + t) * m + p] = scalar_mul_mixed(dev_g1_unchecked(pt), k, bits);
}

__global__ __launch_bounds__(RVBLOCK) void k_rv_sum(RvArgs a, const uint8_t* __restrict__ flags, const G1XYZZ* __restrict__ part,
                                                   G1Affine* __restrict__ pair_pts, uint32_t* __restrict__ k_out) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t m = a.m;
    const uint32_t n_out = a.pok_c ? 4 : 2;
    if (g >= m * n_out) return;
    const uint32_t o = (uint32_t)(g / m);
    const uint64_t p = g % m;
    const bool bad = flags[p] & RV_MALFORMED;
    auto fixed = [&](uint32_t t) { return part[t * m + p]; };
    auto var = [&](uint32_t t) { return part[(a.n_fixed + t) * m + p]; };
    if (o < 2) {
        if (bad) return;                                          // k_rv_miller does not read it
        G1XYZZ acc;
        if (o == 0) {                                             // total_c (kzg10/mod.rs:377-393)
            acc = var(RV_COM_G);
            for (uint32_t t = RV_COM_F; t <= RV_W_W; ++t) add(acc, var(t));
            add(acc, neg(fixed(0)));
            add(acc, neg(fixed(1)));
        } else {                                                  // -total_w (:397)
            acc = G1XYZZ::from_affine(dev_g1_unchecked(a.proofs + 72 * p));
            add(acc, var(RV_TW_GW));
            add(acc, var(RV_TW_W));
            acc = neg(acc);
        }
        pair_pts[o * m + p] = to_affine(acc);
        return;
    }
    uint32_t* out = k_out + 8 * (2 * p + (o - 2));
    if (bad) {
        for (int l = 0; l < 8; ++l) out[l] = 0;
        return;
    }
    // k_0 = s_00 B_0 + s_01 B_1 + c ped_com;  k_1 = Σ s_1j com_f_basis[j] + c com_f  (dlog.rs:135-145)
    G1XYZZ acc = var(RV_N_VAR_KZG + (o - 2));
    const uint32_t lo = o == 2 ? RV_N_FIX_KZG : RV_N_FIX_KZG + 2, hi = o == 2 ? RV_N_FIX_KZG + 2 : RV_N_FIX_KZG + RP_N_RESP;
    for (uint32_t t = lo; t < hi; ++t) add(acc, fixed(t));
    dev_put_g1(to_affine(acc), out, true);
}

__global__ __launch_bounds__(RVBLOCK) void k_rv_miller(const G1Affine* __restrict__ pair_pts, const uint8_t* __restrict__ flags, uint64_t m,
                                                      const EllCoeff* beta_h_c, const EllCoeff* h_c, int beta_h_live, int h_live,
                                                      Fq12* __restrict__ f) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m || (flags[p] & RV_MALFORMED)) return;
    MillerPairs mp;
    mp.p[0] = pair_pts[m + p]; mp.q[0] = G2Affine::inf(); mp.tab[0] = beta_h_c; mp.live[0] = !mp.p[0].is_inf() && beta_h_live;
    mp.p[1] = pair_pts[p]; mp.q[1] = G2Affine::inf(); mp.tab[1] = h_c; mp.live[1] = !mp.p[1].is_inf() && h_live;
    mp.p[2] = G1Affine::inf(); mp.q[2] = G2Affine::inf(); mp.tab[2] = nullptr; mp.live[2] = false;
    f[p] = multi_miller_loop<0>(mp);
}

__global__ __launch_bounds__(RVBLOCK) void k_rv_final(const Fq12* __restrict__ f, const uint8_t* __restrict__ flags, uint64_t m,
                                                     uint8_t* __restrict__ verdict) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const uint32_t fl = flags[p];
    if (fl & RV_MALFORMED) {
        verdict[p] = CG_VERIFY_MALFORMED;
        return;
    }
    Fq12 r;
    const bool some = final_exponentiation(f[p], r);
    const bool ok = some && r == Fq12::one() && (fl & RV_IDENTITY) && (fl & RV_EQ_POS);
    verdict[p] = ok ? CG_VERIFY_ACCEPT : CG_VERIFY_REJECT;
}

// ---- cg_range_verify_proofs_batch: the transcripts either side of the five kernels above --------------------------------
// One lane per showing runs its Merlin transcripts (merlin.hpp), the sponge in LDS at 200 bytes per lane.  Both kernels do
// arithmetic on bytes only and declare no private segment.
//
// In front of k_rv_check: com_f, com_g and com_q compressed as their bytes stand (pts: 3 x 8 words per showing) and the
// range transcript over them -> c, rho.  A point that k_rv_check will refuse gives some c and rho that nothing uses.
__global__ __launch_bounds__(RVBLOCK) void k_rv_challenges(RvArgs a, uint32_t* __restrict__ pts, uint32_t* __restrict__ c, uint32_t* __restrict__ rho) {
    __shared__ __attribute__((aligned(8))) uint8_t sponge[RVBLOCK * ML_STATE];
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.m) return;
    uint32_t* t = pts + 24 * p;
    ml_compress_g1(a.com_f + 16 * p, t);
    ml_compress_g1(a.com_g + 16 * p, t + 8);
    ml_compress_g1(a.com_q + 16 * p, t + 16);
    const uint8_t* b = (const uint8_t*)t;
    ml_range_challenges(sponge + ML_STATE * threadIdx.x, b, b + 32, b + 64, (uint8_t*)(c + 8 * p), (uint8_t*)(rho + 8 * p));
}
// Behind the final exponentiation: the DLEQ's transcript over the slot's bases, k_0, ped_com, com_f_basis, k_1 and com_f
// (dlog.rs:130-169), and `c == self.c` (:171-174): a showing stays CG_VERIFY_ACCEPT only where the challenge equals pok_c.
__global__ __launch_bounds__(RVBLOCK) void k_rv_challenge_dleq(RvArgs a, const uint32_t* __restrict__ pts, const uint32_t* __restrict__ k_pts,
                                                              const uint8_t* __restrict__ slot_bases, const uint8_t* __restrict__ key_bases,
                                                              uint32_t* __restrict__ ped_c, uint32_t* __restrict__ c_dleq, uint8_t* __restrict__ verdict) {
    __shared__ __attribute__((aligned(8))) uint8_t sponge[RVBLOCK * ML_STATE];
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.m || verdict[p] != CG_VERIFY_ACCEPT) return;
    ml_compress_g1(a.ped_com + 16 * p, ped_c + 8 * p);
    ml_range_dleq_challenge(sponge + ML_STATE * threadIdx.x, slot_bases, key_bases, (const uint8_t*)(k_pts + 16 * p),
                            (const uint8_t*)(ped_c + 8 * p), (const uint8_t*)(pts + 24 * p), (uint8_t*)(c_dleq + 8 * p));
    uint32_t differ = 0;
    for (int l = 0; l < 8; ++l) differ |= c_dleq[8 * p + l] ^ a.pok_c[8 * p + l];
    if (differ) verdict[p] = CG_VERIFY_REJECT;
}

// the latency arrangement of the two kernels above (cg_range_vk_set_latency_mode): one workgroup per showing, pairing_team.hpp
__global__ __launch_bounds__(TEAM_WIDTH) void k_rv_lone_miller(const G1Affine* __restrict__ pair_pts, const uint8_t* __restrict__ flags, uint64_t m,
                                                             const EllCoeff* beta_h_c, const EllCoeff* h_c, int beta_h_live, int h_live,
                                                             Fq12* __restrict__ f) {
    __shared__ TeamMem sh;
    const uint64_t p = blockIdx.x;
    // uniform: p is the workgroup's index and flags[p] one byte that every lane of it reads
    if (p >= m || (flags[p] & RV_MALFORMED)) return;
    MillerPairs mp;
    mp.p[0] = pair_pts[m + p]; mp.q[0] = G2Affine::inf(); mp.tab[0] = beta_h_c; mp.live[0] = !mp.p[0].is_inf() && beta_h_live;
    mp.p[1] = pair_pts[p]; mp.q[1] = G2Affine::inf(); mp.tab[1] = h_c; mp.live[1] = !mp.p[1].is_inf() && h_live;
    mp.p[2] = G1Affine::inf(); mp.q[2] = G2Affine::inf(); mp.tab[2] = nullptr; mp.live[2] = false;
    team_miller_to<0>(sh, mp, f + p);
}

__global__ __launch_bounds__(TEAM_WIDTH) void k_rv_lone_final(const Fq12* __restrict__ f, const uint8_t* __restrict__ flags, uint64_t m,
                                                            uint8_t* __restrict__ verdict) {
    __shared__ TeamMem sh;
    const uint64_t p = blockIdx.x;
    if (p >= m) return;                          // uniform: the workgroup's index
    WaveLane ln{(int)threadIdx.x};
    const uint32_t fl = flags[p];
    if (fl & RV_MALFORMED) {                     // uniform: one byte that every lane of the workgroup reads
        if (ln.lane == 0) verdict[p] = CG_VERIFY_MALFORMED;
        return;
    }
    const bool some = team_final_of(sh, ln, f + p);
    const bool ok = some && team_is_one(ln, sh, tp::reg(0)) && (fl & RV_IDENTITY) && (fl & RV_EQ_POS);
    if (ln.lane == 0) verdict[p] = ok ? CG_VERIFY_ACCEPT : CG_VERIFY_REJECT;
}

}  // namespace

struct cg_range_vk : KeyHandle {
    uint32_t n_bits = 0;
    bool latency = false;                  // the pairing stage's arrangement (cg_range_vk_set_latency_mode)
    StageTimer timer;                      // the group stage, the pairing
    RangeConsts kc;
    int h_live = 0, beta_h_live = 0;
    DevBuf<EllCoeff> h_c, beta_h_c;        // prepared h, prepared beta_h
    DevBuf<G1Affine> tab;                  // g, gamma_g, com_f_basis[0..3]
    PedersenSlots slots;                   // per slot: the tables of its two Pedersen bases
    // per-call arrays with their row widths, grown to the largest chunk seen; bytes are the caller's
    RowBuf b_ped{64}, b_comf{64}, b_comg{64}, b_comq{64}, b_evals{96}, b_proofs{288}, b_c{32}, b_rho{32}, b_rz{32}, b_pokc{32},
        b_poks{32 * RP_N_RESP}, b_k{64}, b_flags{1}, b_verdict{1};
    DevBuf<uint32_t> b_scal;               // RV_N_SCALARS per showing, term-major
    DevBuf<G1XYZZ> b_part;                 // one partial per (term, showing)
    DevBuf<G1Affine> b_pair;               // total_c, then -total_w
    DevBuf<Fq12> b_miller;
    // cg_range_verify_proofs_batch: com_f_basis as the DLEQ's transcript absorbs it, 4 x 32 compressed bytes; per showing
    // com_f, com_g, com_q compressed, ped_com compressed and the recomputed c_dleq
    DevBuf<uint8_t> key_cmp;
    RowBuf b_pts{96}, b_pedc{32}, b_cd{32};
    ~cg_range_vk() { drain(); }           // before the buffers above are freed (key_handle.hpp)
};

extern "C" int cg_range_vk_load(cg_range_vk** out, const uint8_t* range_vk_bytes, uint64_t len, uint32_t n_bits, int32_t device) {
    if (!out || !range_vk_bytes) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (int rc = check_range_bits(n_bits, "verify_n_bits")) return rc;
    try {
        // host only: every error of the bytes is reported before any HIP call
        if (len != RV_VK_BYTES)
            throw HipError(CG_ERR_PARSE, "a range proof verifying key is 640 bytes: g, gamma_g, h, beta_h and the four points of com_f_basis");
        KeyRd r{range_vk_bytes, len, 0};
        std::vector<G1Affine> bases(1 + N_TABS, G1Affine::inf());                // build_tables skips the first entry
        bases[1 + TAB_G] = r.g1();
        bases[1 + TAB_GAMMA_G] = r.g1();
        const G2Affine h = r.g2(), beta_h = r.g2();
        for (int i = 0; i < 4; ++i) bases[1 + TAB_CFB + i] = r.g1();
        std::vector<G1Affine> tab;
        build_tables(bases, tab);
        // G2Prepared::from, as the reference's deserialiser computes it (kzg10/data_structures.rs:246-264); O is marked
        std::vector<EllCoeff> h_c(NC), beta_h_c(NC);
        if (!h.is_inf()) g2_prepare(h, h_c.data());
        if (!beta_h.is_inf()) g2_prepare(beta_h, beta_h_c.data());
        std::unique_ptr<cg_range_vk> k(new cg_range_vk());
        k->n_bits = n_bits;
        k->kc = range_consts((uint32_t)ilog2_ceil(n_bits));
        k->h_live = !h.is_inf();
        k->beta_h_live = !beta_h.is_inf();
        k->open(device);
        k->timer.create();
        k->tab.alloc(tab.size());
        h2d_sync(k->tab.p, tab.data(), tab.size() * sizeof(G1Affine), k->st);
        k->h_c.alloc(NC);
        k->beta_h_c.alloc(NC);
        h2d_sync(k->h_c.p, h_c.data(), NC * sizeof(EllCoeff), k->st);
        h2d_sync(k->beta_h_c.p, beta_h_c.data(), NC * sizeof(EllCoeff), k->st);
        uint32_t key_cmp[4 * 8];
        for (int i = 0; i < 4; ++i) {
            uint32_t w[16];
            memcpy(w, range_vk_bytes + RV_VK_BYTES - 256 + 64 * i, 64);
            ml_compress_g1(w, key_cmp + 8 * i);
        }
        k->key_cmp.alloc(sizeof(key_cmp));
        h2d_sync(k->key_cmp.p, key_cmp, sizeof(key_cmp), k->st);
        *out = k.release();
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}

extern "C" int cg_range_vk_add_bases(cg_range_vk* k, const uint8_t ped_bases[128], uint32_t* slot) {
    if (!k || !ped_bases || !slot) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    return k->slots.add(*k, ped_bases, slot);
}

extern "C" void cg_range_vk_free(cg_range_vk* k) { free_handle(k); }

extern "C" int cg_range_vk_set_latency_mode(cg_range_vk* k, int32_t on) { return set_latency_mode(k, on); }

// Diagnostic: what the kernels of the handle's last call took, by HIP events, summed over its chunks: the group stage
// (k_rv_check, k_rv_terms, k_rv_sum) and the pairing (k_rv_miller, k_rv_final)
extern "C" int cg_range_vk_last_kernel_ms(cg_range_vk* k, float* group_ms, float* pairing_ms) { return last_kernel_ms(k, group_ms, pairing_ms); }

namespace {
// one call's arrays on the host, as the caller laid them out; which of them may be null depends on the entry
struct RvHost {
    const uint8_t *ped_com, *com_f, *com_g, *com_q, *evals, *proofs, *c, *rho, *randomizers, *pok_c, *pok_s;
};

void rv_reserve(cg_range_vk* k, uint64_t chunk) {
    for (RowBuf* b : {&k->b_ped, &k->b_comf, &k->b_comg, &k->b_comq, &k->b_evals, &k->b_proofs, &k->b_c, &k->b_rho, &k->b_rz, &k->b_pokc,
                      &k->b_poks, &k->b_k, &k->b_flags, &k->b_verdict, &k->b_pts, &k->b_pedc, &k->b_cd})
        b->reserve(chunk);
    grow(k->b_scal, chunk * 8 * RV_N_SCALARS);
    grow(k->b_part, chunk * (uint64_t)(RV_N_FIX_KZG + N_FIX_DLEQ + RV_N_VAR_KZG + N_VAR_DLEQ));
    grow(k->b_pair, chunk * 2);
    grow(k->b_miller, chunk);
}

// One chunk of either verifying entry on the key's stream: rows [off, off + m) go up, the kernels follow; nothing comes
// down and nothing waits.  own_transcripts (cg_range_verify_proofs_batch): c and rho are derived in front of the five
// kernels and the DLEQ's challenge is recomputed and compared behind them.  d_ped_com, where given, is ped_com on the
// device already, and d_verdicts, where given, takes the verdict bytes instead of the key's own array.
void rv_chunk(cg_range_vk* k, bool own_transcripts, uint32_t slot, const G1Affine* tab_slot, const RvHost& h, uint64_t off, uint64_t m,
              const uint32_t* d_ped_com, uint8_t* d_verdicts) {
    const bool pok = h.pok_c != nullptr;
    const uint32_t n_fixed = RV_N_FIX_KZG + (pok ? N_FIX_DLEQ : 0), n_var = RV_N_VAR_KZG + (pok ? N_VAR_DLEQ : 0);
    uint8_t* verdict = d_verdicts ? d_verdicts : k->b_verdict.bytes();
    if (pok) {
        if (!d_ped_com) k->b_ped.up(k->st, h.ped_com, off, m);
        k->b_pokc.up(k->st, h.pok_c, off, m);
        k->b_poks.up(k->st, h.pok_s, off, m);
    }
    k->b_comf.up(k->st, h.com_f, off, m);
    k->b_comg.up(k->st, h.com_g, off, m);
    k->b_comq.up(k->st, h.com_q, off, m);
    k->b_evals.up(k->st, h.evals, off, m);
    k->b_proofs.up(k->st, h.proofs, off, m);
    if (!own_transcripts) {
        k->b_c.up(k->st, h.c, off, m);
        k->b_rho.up(k->st, h.rho, off, m);
    }
    k->b_rz.up(k->st, h.randomizers, off, m);
    const RvArgs a{d_ped_com ? d_ped_com : k->b_ped.words(), k->b_comf.words(), k->b_comg.words(), k->b_comq.words(), k->b_evals.words(),
                   k->b_proofs.words(), k->b_c.words(), k->b_rho.words(), k->b_rz.words(), pok ? k->b_pokc.words() : nullptr,
                   pok ? k->b_poks.words() : nullptr, m, n_fixed, n_var};
    const uint32_t grid = ceil_div(m, RVBLOCK);
    k->timer.mark(0, k->st);
    if (own_transcripts) {
        k_rv_challenges<<<grid, RVBLOCK, 0, k->st>>>(a, k->b_pts.words_mut(), k->b_c.words_mut(), k->b_rho.words_mut());
        CG_KERNEL_CHECK();
    }
    k_rv_check<<<grid, RVBLOCK, 0, k->st>>>(k->kc, a, k->b_scal.p, k->b_flags.bytes());
    CG_KERNEL_CHECK();
    k_rv_terms<<<ceil_div(m * n_fixed, RVBLOCK) + ceil_div(m * n_var, RVBLOCK), RVBLOCK, 0, k->st>>>(
        a, k->b_scal.p, k->b_flags.bytes(), k->tab.p, tab_slot, k->b_part.p);
    CG_KERNEL_CHECK();
    k_rv_sum<<<ceil_div(m * (pok ? 4 : 2), RVBLOCK), RVBLOCK, 0, k->st>>>(a, k->b_flags.bytes(), k->b_part.p, k->b_pair.p, k->b_k.words_mut());
    CG_KERNEL_CHECK();
    k->timer.mark(1, k->st);
    if (k->latency) {
        k_rv_lone_miller<<<(uint32_t)m, TEAM_WIDTH, 0, k->st>>>(k->b_pair.p, k->b_flags.bytes(), m, k->beta_h_c.p, k->h_c.p, k->beta_h_live,
                                                               k->h_live, k->b_miller.p);
        CG_KERNEL_CHECK();
        k_rv_lone_final<<<(uint32_t)m, TEAM_WIDTH, 0, k->st>>>(k->b_miller.p, k->b_flags.bytes(), m, verdict);
    } else {
        k_rv_miller<<<grid, RVBLOCK, 0, k->st>>>(k->b_pair.p, k->b_flags.bytes(), m, k->beta_h_c.p, k->h_c.p, k->beta_h_live, k->h_live, k->b_miller.p);
        CG_KERNEL_CHECK();
        k_rv_final<<<grid, RVBLOCK, 0, k->st>>>(k->b_miller.p, k->b_flags.bytes(), m, verdict);
    }
    CG_KERNEL_CHECK();
    if (own_transcripts) {
        k_rv_challenge_dleq<<<grid, RVBLOCK, 0, k->st>>>(a, k->b_pts.words(), k->b_k.words(), k->slots.compressed(slot), k->key_cmp.p,
                                                         k->b_pedc.words_mut(), k->b_cd.words_mut(), verdict);
        CG_KERNEL_CHECK();
    }
    k->timer.mark(2, k->st);
}

// Both public verifying entries: the chunks one after the other, each waited for before its verdicts are the caller's
int run_range_verify(cg_range_vk* k, bool own_transcripts, uint32_t slot, const RvHost& h, uint64_t n, uint8_t* verdicts, uint8_t* k_out) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    try {
        std::lock_guard<std::mutex> lk(k->mu);
        const G1Affine* tab_slot = k->slots.table(slot, "cg_range_vk_add_bases");
        if (n == 0) return CG_OK;
        const bool pok = h.pok_c != nullptr;
        if (!h.com_f || !h.com_g || !h.com_q || !h.evals || !h.proofs || !h.randomizers || !verdicts || (pok && (!h.ped_com || !h.pok_s)) ||
            (own_transcripts ? !pok : !h.c || !h.rho || (pok && !k_out)))
            return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
        CG_HIP(hipSetDevice(k->device));
        const uint64_t chunk = n < RVCHUNK ? n : RVCHUNK;
        rv_reserve(k, chunk);
        k->timer.reset();
        for (uint64_t off = 0; off < n; off += chunk) {
            const uint64_t m = n - off < chunk ? n - off : chunk;
            rv_chunk(k, own_transcripts, slot, tab_slot, h, off, m, nullptr, nullptr);
            k->b_verdict.down(k->st, verdicts, off, m);
            if (pok && !own_transcripts) k->b_k.down(k->st, k_out, off, m);
            CG_HIP(hipStreamSynchronize(k->st));
            k->timer.add();
        }
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}
}  // namespace

// ---- the internal entry (rangeverify.hpp): what cg_verify_showings_batch needs of a range key it did not load ------------
namespace cg {
std::mutex& range_vk_lock(cg_range_vk* k) { return k->mu; }
int range_vk_device(const cg_range_vk* k) { return k->device; }
hipStream_t range_vk_stream(cg_range_vk* k) { return k->st; }
const uint8_t* range_vk_slot_bytes(const cg_range_vk* k, uint32_t slot) {
    return slot < k->slots.registered.size() ? k->slots.registered[slot].data() : nullptr;
}
void range_vk_reserve(cg_range_vk* k, uint64_t chunk) {
    rv_reserve(k, chunk);
    k->timer.reset();                     // the stages of such a call interleave with another handle's: nothing is timed
}
void range_vk_enqueue(cg_range_vk* k, uint32_t slot, const cg_range_rows& rows, uint64_t off, uint64_t m, const uint32_t* d_ped_com,
                      uint8_t* d_verdicts) {
    const RvHost h{nullptr, rows.com_f, rows.com_g, rows.com_q, rows.evals, rows.proofs, nullptr, nullptr, rows.randomizers, rows.pok_c, rows.pok_s};
    rv_chunk(k, true, slot, k->slots.table(slot, "cg_range_vk_add_bases"), h, off, m, d_ped_com, d_verdicts);
}
}  // namespace cg

extern "C" int cg_range_verify_batch(cg_range_vk* k, uint32_t slot, const uint8_t* ped_com, const uint8_t* com_f, const uint8_t* com_g,
                                     const uint8_t* com_q, const uint8_t* evals, const uint8_t* proofs, const uint8_t* c,
                                     const uint8_t* rho, const uint8_t* randomizers, const uint8_t* pok_c, const uint8_t* pok_s,
                                     uint64_t n, uint8_t* verdicts, uint8_t* k_out) {
    return run_range_verify(k, false, slot, RvHost{ped_com, com_f, com_g, com_q, evals, proofs, c, rho, randomizers, pok_c, pok_s}, n, verdicts, k_out);
}

// `verify_n_bits` whole: CG_VERIFY_ACCEPT is exactly `verify_n_bits(..) == true`
extern "C" int cg_range_verify_proofs_batch(cg_range_vk* k, uint32_t slot, const uint8_t* ped_com, const uint8_t* com_f, const uint8_t* com_g,
                                            const uint8_t* com_q, const uint8_t* evals, const uint8_t* proofs, const uint8_t* randomizers,
                                            const uint8_t* pok_c, const uint8_t* pok_s, uint64_t n, uint8_t* verdicts) {
    return run_range_verify(k, true, slot, RvHost{ped_com, com_f, com_g, com_q, evals, proofs, nullptr, nullptr, randomizers, pok_c, pok_s}, n,
                            verdicts, nullptr);
}
