// Creating range proofs on the GPU: `ClientState::show_range` -> `RangeProof::prove_n_bits` (creds/src/rangeproof.rs:114-339)
// for a batch of Pedersen openings under one KZG key, up to the three Merlin transcripts, which stay with the host, and
// with every random scalar given by the caller.
//
// A cg_range_pk holds, on a device, fixed-base tables (fixed_base.hpp: 32 windows x 256 multiples) of powers_of_g[0..2n+3]
// and powers_of_gamma_g[0..3] - the only powers prove_n_bits reaches: deg q = deg w^ = 2n + 3 - and, per registered slot,
// of one pair of Pedersen bases.  Each of the three calls is stateless and runs three kernels per chunk of showings on the
// handle's own non-blocking stream (a kernel pair, k_range_terms and k_range_sum, makes the points):
//   k_range_poly    one wave per showing: the polynomial stage (rangepoly.hpp) with its vectors in LDS, lanes taking output
//                   coefficients; the checks that make a showing CG_SHOW_MALFORMED; the scalar of every fixed-base term,
//                   canonical, and in the open call the evaluations and the random_v
//   k_range_terms   one lane per (showing, term): the term's scalar times its base by the 32-addition walk of fixed_base.hpp.
//                   This is the hot path: 263 walks per proof at n = 32, the lanes of every wave but the last all busy
//   k_range_sum     one lane per (showing, output point): the point's XYZZ partials summed with the general `add` (chosen
//                   randomness makes partials coincide or cancel), affine, written as ark-serialize writes it
// This is the arrangement of cg_show_commit_batch.  A fused kernel - one wave per (showing, point), the partials summed in a
// tree through LDS and none of them in HBM - was built and measured beside it and lost: a point's 4, 2, 39, 69 or 71 terms
// leave 38 - 56 % of such a wave's lanes walking, against all of them here (profiles/range_create.md).
//   commit    com_f, com_g, k_0, k_1          n + 17 terms     (KZG10::commit, kzg10/mod.rs:178-241; dlog.rs:60-91)
//   quotient  com_q                           2n + 7 terms     (rangeproof.rs:260-268)
//   open      W of proof_g, proof_gw, proof_w^   4n + 15 terms (KZG10::open, kzg10/mod.rs:247-331)
// cg_range_respond_batch, the DLEQ's responses once the host's transcript has produced its challenge, is host arithmetic.
// cg_range_prove_batch is the three phases in one call with the transcripts on the device (merlin.hpp): the same kernels,
// k_range_challenge_c and k_range_challenge_rho between them and k_range_finish (the responses) behind them.  Its chunk
// body is also rangeproof.hpp's internal entry, which cg_create_showings_batch (verify.hip) puts behind its own kernels.
// The handle's device, stream and lock, the timing of the two stages, the slots and the per-call arrays are key_handle.hpp's
// (KeyHandle, StageTimer, PedersenSlots, RowBuf), shared with cg_pvk and cg_range_vk; so are the responses (dlog_respond).
#include <memory>

#include "common.hpp"
#include "fixed_base.hpp"
#include "key_handle.hpp"
#include "rangepoly.hpp"
#include "rangeproof.hpp"

using namespace cg;

namespace {

constexpr uint64_t RCHUNK = 1u << 12;      // showings per launch set: 4n + 15 term scalars each in the open call
constexpr int RWAVE = 64;
constexpr uint32_t RP_SLOT = 0x80000000u;  // in tab_of: a table of the call's slot (0 or 1) instead of the key's
enum { PH_COMMIT = 0, PH_QUOTIENT = 1, PH_OPEN = 2 };

// One output point: terms [term0, term0 + n_terms) of a showing.  It goes to the showing's row of uncompressed buffer
// `unc_buf` at word unc_at and / or to its row of the compressed buffer at word cmp_at (-1: not written).
struct RpPoint {
    uint32_t term0, n_terms;
    int32_t unc_buf, unc_at, cmp_at;
};
struct RpShape {
    uint32_t n_pts, n_terms;               // per showing
    uint32_t unc_words[2], cmp_words;      // a showing's row in each output buffer
    RpPoint pt[4];
};

struct WaveLane {
    int lane;
    static constexpr int nl = RWAVE;
    __device__ void sync() const { __syncthreads(); }
};

template <int PHASE>
__global__ __launch_bounds__(RWAVE) void k_range_poly(RangeConsts kc, const uint32_t* __restrict__ open, const uint32_t* __restrict__ rand,
                                                     const uint32_t* __restrict__ c, const uint32_t* __restrict__ rho, uint64_t n,
                                                     uint32_t n_terms, uint32_t* __restrict__ terms, uint32_t* __restrict__ evals,
                                                     uint32_t* __restrict__ proofs, uint8_t* __restrict__ status, int chained) {
    __shared__ RangeWork W;
    const uint64_t p = blockIdx.x;
    if (p >= n) return;
    WaveLane ln{(int)threadIdx.x};
    const RangeIn in{open + 16 * p, rand + 8 * RP_N_RAND * p, PHASE >= PH_QUOTIENT ? c + 8 * p : nullptr, PHASE == PH_OPEN ? rho + 8 * p : nullptr};
    uint32_t* t = terms + 8 * p * n_terms;
    bool made;                                                    // the same in every lane: it depends on the inputs alone
    // chained (cg_range_prove_batch): a showing that an earlier phase of the same call refused stays refused.  One byte
    // that every lane of the workgroup reads, and that only lane 0 writes, at the end
    if (chained && status[p] != CG_SHOW_MADE) made = false;
    else if (PHASE == PH_COMMIT) made = rp_commit(kc, in, W, t, ln);
    else if (PHASE == PH_QUOTIENT) made = rp_quotient_call(kc, in, W, t, ln);
    else made = rp_open(kc, in, W, t, evals + 24 * p, proofs + 72 * p, ln);
    if (ln.lane == 0) status[p] = made ? CG_SHOW_MADE : CG_SHOW_MALFORMED;
    if (PHASE == PH_OPEN && !made && ln.lane < 24) {
        evals[24 * p + ln.lane] = 0;
        proofs[72 * p + 24 * (ln.lane >> 3) + 16 + (ln.lane & 7)] = 0;
    }
}

// one lane per (showing, term): the term's scalar times its base, from the table; nothing for a malformed showing
__global__ __launch_bounds__(RWAVE) void k_range_terms(const RpShape* __restrict__ shape, const uint32_t* __restrict__ tab_of,
                                                      const uint32_t* __restrict__ terms, const G1Affine* __restrict__ tab,
                                                      const G1Affine* __restrict__ tab_slot, const uint8_t* __restrict__ status,
                                                      uint64_t n, G1XYZZ* __restrict__ part) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nt = shape->n_terms;
    if (g >= n * nt) return;
    if (status[g / nt] != CG_SHOW_MADE) return;
    const uint32_t of = tab_of[g % nt];
    const G1Affine* tb = of & RP_SLOT ? tab_slot + (uint64_t)(of & ~RP_SLOT) * FB_NWIN * FB_WIN : tab + (uint64_t)of * FB_NWIN * FB_WIN;
    part[g] = fixed_base_mul(tb, terms + 8 * g);
}
// one lane per (showing, output point): the partials summed with the general `add` (chosen randomness makes partials
// coincide or cancel), affine, written as ark-serialize writes them; zeros for a malformed showing
__global__ __launch_bounds__(RWAVE) void k_range_sum(const RpShape* __restrict__ shape, const uint8_t* __restrict__ status,
                                                    uint64_t n, const G1XYZZ* __restrict__ part, uint32_t* __restrict__ unc0,
                                                    uint32_t* __restrict__ unc1, uint32_t* __restrict__ cmp) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n_pts = shape->n_pts;
    if (g >= n * n_pts) return;
    const uint64_t p = g / n_pts;
    const RpPoint* sg = &shape->pt[g % n_pts];
    const bool made = status[p] == CG_SHOW_MADE;
    uint32_t* u = sg->unc_buf < 0 ? nullptr : (sg->unc_buf ? unc1 : unc0) + p * shape->unc_words[sg->unc_buf] + sg->unc_at;
    uint32_t* cw = sg->cmp_at < 0 ? nullptr : cmp + p * shape->cmp_words + sg->cmp_at;
    if (!made) {
        if (u) for (int l = 0; l < 16; ++l) u[l] = 0;
        if (cw) for (int l = 0; l < 8; ++l) cw[l] = 0;
        return;
    }
    G1XYZZ acc = G1XYZZ::inf();
    for (uint32_t j = 0; j < sg->n_terms; ++j) add(acc, part[p * shape->n_terms + sg->term0 + j]);
    const G1Affine a = to_affine(acc);
    if (u) dev_put_g1(a, u, false);
    if (cw) dev_put_g1(a, cw, true);
}

// ---- cg_range_prove_batch: the transcripts between the phases, and the end ---------------------------------------------
// One lane per showing runs its Merlin transcripts (merlin.hpp), the sponge in LDS at 200 bytes per lane.  Both kernels do
// arithmetic on bytes only - no field multiplication, whose call would bring a stack - and declare no private segment.
// A showing that is not CG_SHOW_MADE gets zero challenges; the phases after it skip it.
//
// After the commit phase: c from the range transcript over com_f, com_g (ts: the phase's four compressed points) and
// c_dleq from the DLEQ's over the slot's and the key's compressed bases, k_0, k_1, ped_com and com_f.  ped_com is
// compressed here as its bytes stand; k_range_finish refuses a showing whose ped_com is no valid point.
__global__ __launch_bounds__(RWAVE) void k_range_challenge_c(const uint32_t* __restrict__ ts, const uint32_t* __restrict__ ped,
                                                            const uint8_t* __restrict__ slot_bases, const uint8_t* __restrict__ key_bases,
                                                            const uint8_t* __restrict__ status, uint64_t n, uint32_t* __restrict__ ped_c,
                                                            uint32_t* __restrict__ c, uint32_t* __restrict__ c_dleq) {
    __shared__ __attribute__((aligned(8))) uint8_t sponge[RWAVE * ML_STATE];
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (status[p] != CG_SHOW_MADE) {
        for (int l = 0; l < 8; ++l) c[8 * p + l] = c_dleq[8 * p + l] = 0;
        return;
    }
    uint8_t* st = sponge + ML_STATE * threadIdx.x;
    const uint8_t* t = (const uint8_t*)(ts + 32 * p);
    ml_compress_g1(ped + 16 * p, ped_c + 8 * p);
    ml_range_challenges(st, t, t + 32, nullptr, (uint8_t*)(c + 8 * p), nullptr);
    ml_range_dleq_challenge(st, slot_bases, key_bases, t + 64, (const uint8_t*)(ped_c + 8 * p), t, (uint8_t*)(c_dleq + 8 * p));
}
// After the quotient phase: rho, the range transcript replayed from its start with com_q (ts_q) appended.
__global__ __launch_bounds__(RWAVE) void k_range_challenge_rho(const uint32_t* __restrict__ ts, const uint32_t* __restrict__ ts_q,
                                                              const uint8_t* __restrict__ status, uint64_t n, uint32_t* __restrict__ rho) {
    __shared__ __attribute__((aligned(8))) uint8_t sponge[RWAVE * ML_STATE];
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (status[p] != CG_SHOW_MADE) {
        for (int l = 0; l < 8; ++l) rho[8 * p + l] = 0;
        return;
    }
    const uint8_t* t = (const uint8_t*)(ts + 32 * p);
    ml_range_challenges(sponge + ML_STATE * threadIdx.x, t, t + 32, (const uint8_t*)(ts_q + 8 * p), nullptr, (uint8_t*)(rho + 8 * p));
}

// what cg_range_prove_batch hands back, one row per showing in each array
struct RpProof {
    uint32_t *com_f, *com_g, *com_q;       // 16 words
    uint32_t *evals, *proofs;              // 24, 72
    uint32_t *pok_c, *pok_s;               // 8, 48
    uint32_t* challenges;                  // 24: c_dleq, c, rho
};
// The end of a proof, one lane per showing: ped_com's checked deserialisation, the DLEQ's responses s = nonce - c_dleq *
// secret (dlog.rs:101-109; every scalar was found below r by the commit phase) and the three challenges side by side.
// A showing that any phase refused, or whose ped_com is refused here, has EVERY output row zeroed, those that earlier
// phases wrote included.  The one condition that can first appear after the commit phase is rho^n_bits = 1 for the rho
// the transcript gave: no input is known that provokes it through the hash, so no test reaches it, and it is right by
// construction: the open phase sets the status, and the status alone decides here.
__global__ __launch_bounds__(RWAVE) void k_range_finish(const uint32_t* __restrict__ open, const uint32_t* __restrict__ rand,
                                                       const uint32_t* __restrict__ ped, const uint32_t* __restrict__ c,
                                                       const uint32_t* __restrict__ rho, uint64_t n, RpProof o, uint8_t* __restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    bool made = status[p] == CG_SHOW_MADE;
    (void)dev_g1(ped + 16 * p, made);
    if (!made) {
        status[p] = CG_SHOW_MALFORMED;
        for (int l = 0; l < 16; ++l) o.com_f[16 * p + l] = o.com_g[16 * p + l] = o.com_q[16 * p + l] = 0;
        for (int l = 0; l < 24; ++l) o.evals[24 * p + l] = o.challenges[24 * p + l] = 0;
        for (int l = 0; l < 72; ++l) o.proofs[72 * p + l] = 0;
        for (int l = 0; l < 8; ++l) o.pok_c[8 * p + l] = 0;
        for (int l = 0; l < 48; ++l) o.pok_s[48 * p + l] = 0;
        return;
    }
    static constexpr int8_t SECRET[RP_N_RESP] = {-1, -2, RP_F, RP_F + 1, RP_F + 2, -1};     // -1: m, -2: r, else a rand index
    static constexpr int8_t NONCE[RP_N_RESP] = {RP_TM, RP_TR, RP_TF, RP_TF + 1, RP_TF + 2, RP_TM};
    const uint32_t* rd = rand + 8 * RP_N_RAND * p;
    const Fr cm = to_mont(dev_fr(o.pok_c + 8 * p));                // c·R times a canonical x is c·x, canonical
    for (int t = 0; t < RP_N_RESP; ++t) {
        const Fr secret = dev_fr(SECRET[t] < 0 ? open + 16 * p + 8 * (-1 - SECRET[t]) : rd + 8 * SECRET[t]);
        rp_store(o.pok_s + 48 * p + 8 * t, sub(dev_fr(rd + 8 * NONCE[t]), mul(cm, secret)));
    }
    for (int l = 0; l < 8; ++l) {
        o.challenges[24 * p + l] = o.pok_c[8 * p + l];
        o.challenges[24 * p + 8 + l] = c[8 * p + l];
        o.challenges[24 * p + 16 + l] = rho[8 * p + l];
    }
}

// the three calls' layouts for a domain of n: which table every term walks (the order rangepoly.hpp writes the scalars
// in) and which terms make which point.  Tables 0..2n+3 are powers_of_g's, 2n+4..2n+7 powers_of_gamma_g's.
void range_shapes(uint32_t n, RpShape sh[3], std::vector<uint32_t> tab_of[3]) {
    const uint32_t G0 = 0, GAM = 2 * n + 4;
    auto powers = [&](std::vector<uint32_t>& v, uint32_t n_g, uint32_t n_gam) {
        for (uint32_t i = 0; i < n_g; ++i) v.push_back(G0 + i);
        for (uint32_t i = 0; i < n_gam; ++i) v.push_back(GAM + i);
    };
    memset(sh, 0, 3 * sizeof(RpShape));
    // commit: m f0 f1 f2 | g~ (n + 3), g0..g3 | t_m t_r | t_f0 t_f1 t_f2 t_m  ->  com_f, com_g, k_0, k_1
    std::vector<uint32_t>& t0 = tab_of[PH_COMMIT];
    t0 = {G0, GAM, GAM + 1, GAM + 2};
    powers(t0, n + 3, 4);
    t0.insert(t0.end(), {RP_SLOT | 0u, RP_SLOT | 1u, GAM, GAM + 1, GAM + 2, G0});
    sh[PH_COMMIT] = {4, rp_commit_terms(n), {16, 16}, 32,
                     {{0, 4, 0, 0, 0}, {4, n + 7, 1, 0, 8}, {n + 11, 2, -1, 0, 16}, {n + 13, 4, -1, 0, 24}}};
    // quotient: q (2n + 4), q0 q1 q2  ->  com_q
    powers(tab_of[PH_QUOTIENT], 2 * n + 4, 3);
    sh[PH_QUOTIENT] = {1, rp_quotient_terms(n), {16, 0}, 8, {{0, 2 * n + 7, 0, 0, 0}}};
    // open: per proof the witness quotient, then the blinded one; a proof is W (16 words) ‖ random_v (8)
    powers(tab_of[PH_OPEN], n + 2, 3);
    powers(tab_of[PH_OPEN], n + 2, 3);
    powers(tab_of[PH_OPEN], 2 * n + 3, 2);
    sh[PH_OPEN] = {3, rp_open_terms(n), {72, 0}, 0, {{0, n + 5, 0, 0, -1}, {n + 5, n + 5, 0, 24, -1}, {2 * n + 10, 2 * n + 5, 0, 48, -1}}};
    for (int ph = 0; ph < 3; ++ph)
        if (tab_of[ph].size() != sh[ph].n_terms) throw HipError(CG_ERR_HIP, "internal: range proof term layout");
}

}  // namespace

struct cg_range_pk : KeyHandle {
    uint32_t n_bits = 0;
    StageTimer timer;                      // the polynomial stage, the points
    RangeConsts kc;
    RpShape shape[3];
    DevBuf<G1Affine> tab;                  // powers_of_g[0..2n+3], then powers_of_gamma_g[0..3]
    PedersenSlots slots;                   // per slot: the tables of its two Pedersen bases
    DevBuf<RpShape> d_shape;               // the three calls' layouts
    DevBuf<uint32_t> d_tab_of[3];
    // per-call arrays with their row widths (a call's layout sets the others), grown to the largest chunk seen; bytes are
    // the caller's
    RowBuf b_open{64}, b_rand{32 * RP_N_RAND}, b_c{32}, b_rho{32}, b_terms, b_unc0, b_unc1, b_cmp, b_evals, b_status{1};
    DevBuf<G1XYZZ> b_part;                 // one partial per (showing, term)
    // cg_range_prove_batch: com_f_basis (gamma_g[0..2], g[0]) as the DLEQ's transcript absorbs it, 4 x 32 compressed bytes,
    // and the call's own arrays, which hold a chunk's proofs from the phase that writes them to the one copy down
    DevBuf<uint8_t> key_cmp;
    RowBuf o_ped{64}, o_pedc{32}, o_comf{64}, o_comg{64}, o_ts{128}, o_comq{64}, o_tsq{32}, o_evals{96}, o_proofs{288}, o_pokc{32},
        o_poks{32 * RP_N_RESP}, o_chal{96};
    ~cg_range_pk() { drain(); }            // before the buffers above are freed (key_handle.hpp)
};

extern "C" int cg_range_pk_load(cg_range_pk** out, const uint8_t* range_pk_bytes, uint64_t len, uint32_t n_bits, int32_t device) {
    if (!out || !range_pk_bytes) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (int rc = check_range_bits(n_bits, "prove_n_bits")) return rc;
    try {
        // host only: every error of the bytes is reported before any HIP call
        KeyRd r{range_pk_bytes, len, 0};
        std::vector<G1Affine> pg(r.count(64)), bases(1, G1Affine::inf());
        for (G1Affine& p : pg) p = r.g1();
        std::vector<G1Affine> pgam(r.count(64));
        for (G1Affine& p : pgam) p = r.g1();
        if (r.off != len) throw HipError(CG_ERR_PARSE, "trailing bytes after the powers of a range proof key");
        const uint32_t n = n_bits;
        if (pg.size() < 2 * n + 4 || pgam.size() < 4)
            return fail(CG_ERR_MALFORMED_KEY, "%llu powers of g and %llu of gamma_g: proofs of %u bits take %u and 4",
                        (unsigned long long)pg.size(), (unsigned long long)pgam.size(), n, 2 * n + 4);
        bases.insert(bases.end(), pg.begin(), pg.begin() + 2 * n + 4);         // build_tables skips the first entry
        bases.insert(bases.end(), pgam.begin(), pgam.begin() + 4);
        std::vector<G1Affine> tab;
        build_tables(bases, tab);
        uint32_t key_cmp[4 * 8];                                               // gamma_g[0..2], then g[0]: com_f_basis
        for (int i = 0; i < 4; ++i) {
            uint32_t w[16];
            memcpy(w, range_pk_bytes + (i < 3 ? 16 + 64 * pg.size() + 64 * i : 8), 64);
            ml_compress_g1(w, key_cmp + 8 * i);
        }
        std::unique_ptr<cg_range_pk> k(new cg_range_pk());
        k->n_bits = n;
        k->kc = range_consts((uint32_t)ilog2_ceil(n));
        std::vector<uint32_t> tab_of[3];
        range_shapes(n, k->shape, tab_of);
        k->open(device);
        k->timer.create();
        k->tab.alloc(tab.size());
        h2d_sync(k->tab.p, tab.data(), tab.size() * sizeof(G1Affine), k->st);
        k->key_cmp.alloc(sizeof(key_cmp));
        h2d_sync(k->key_cmp.p, key_cmp, sizeof(key_cmp), k->st);
        k->d_shape.alloc(3);
        h2d_sync(k->d_shape.p, k->shape, 3 * sizeof(RpShape), k->st);
        for (int ph = 0; ph < 3; ++ph) {
            k->d_tab_of[ph].alloc(tab_of[ph].size());
            h2d_sync(k->d_tab_of[ph].p, tab_of[ph].data(), tab_of[ph].size() * sizeof(uint32_t), k->st);
        }
        *out = k.release();
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}

extern "C" int cg_range_pk_add_bases(cg_range_pk* k, const uint8_t ped_bases[128], uint32_t* slot) {
    if (!k || !ped_bases || !slot) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    return k->slots.add(*k, ped_bases, slot);
}

extern "C" void cg_range_pk_free(cg_range_pk* k) { free_handle(k); }

// Diagnostic: what the two kernels of the handle's last GPU call took, by HIP events, summed over its chunks
extern "C" int cg_range_pk_last_kernel_ms(cg_range_pk* k, float* poly_ms, float* points_ms) { return last_kernel_ms(k, poly_ms, points_ms); }

namespace {
struct RpCall {
    int phase;
    uint32_t slot;
    const uint8_t *open, *rand, *c, *rho;
    uint64_t n;
    uint8_t *unc0, *unc1, *cmp, *evals, *status;
};

int run_range(cg_range_pk* k, const RpCall& a) {
    try {
        std::lock_guard<std::mutex> lk(k->mu);
        const G1Affine* tab_slot = a.phase == PH_COMMIT ? k->slots.table(a.slot, "cg_range_pk_add_bases") : nullptr;
        if (a.n == 0) return CG_OK;
        const bool null_in = !a.open || !a.rand || (a.phase >= PH_QUOTIENT && !a.c) || (a.phase == PH_OPEN && !a.rho);
        const bool null_out = !a.unc0 || !a.status || (a.phase == PH_COMMIT && !a.unc1) || (a.phase != PH_OPEN && !a.cmp) || (a.phase == PH_OPEN && !a.evals);
        if (null_in || null_out) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
        CG_HIP(hipSetDevice(k->device));
        const RpShape& sh = k->shape[a.phase];
        const uint64_t chunk = a.n < RCHUNK ? a.n : RCHUNK;
        for (RowBuf* b : {&k->b_open, &k->b_rand, &k->b_c, &k->b_rho, &k->b_status}) b->reserve(chunk);
        k->b_terms.reserve(chunk, 32 * sh.n_terms);
        k->b_unc0.reserve(chunk, 4 * sh.unc_words[0]);
        k->b_unc1.reserve(chunk, 4 * sh.unc_words[1]);
        k->b_cmp.reserve(chunk, 4 * sh.cmp_words);
        k->b_evals.reserve(chunk, a.phase == PH_OPEN ? 96 : 0);
        grow(k->b_part, chunk * sh.n_terms);
        k->timer.reset();
        for (uint64_t off = 0; off < a.n; off += chunk) {
            const uint64_t m = a.n - off < chunk ? a.n - off : chunk;
            k->b_open.up(k->st, a.open, off, m);
            k->b_rand.up(k->st, a.rand, off, m);
            if (a.phase >= PH_QUOTIENT) k->b_c.up(k->st, a.c, off, m);
            if (a.phase == PH_OPEN) k->b_rho.up(k->st, a.rho, off, m);
            const uint32_t *d_open = k->b_open.words(), *d_rand = k->b_rand.words(), *d_c = k->b_c.words(), *d_rho = k->b_rho.words();
            uint32_t *d_terms = k->b_terms.words_mut(), *d_ev = k->b_evals.words_mut(), *d_u0 = k->b_unc0.words_mut();
            k->timer.mark(0, k->st);
            if (a.phase == PH_COMMIT)
                k_range_poly<PH_COMMIT><<<(uint32_t)m, RWAVE, 0, k->st>>>(k->kc, d_open, d_rand, d_c, d_rho, m, sh.n_terms, d_terms, d_ev, d_u0, k->b_status.bytes(), 0);
            else if (a.phase == PH_QUOTIENT)
                k_range_poly<PH_QUOTIENT><<<(uint32_t)m, RWAVE, 0, k->st>>>(k->kc, d_open, d_rand, d_c, d_rho, m, sh.n_terms, d_terms, d_ev, d_u0, k->b_status.bytes(), 0);
            else
                k_range_poly<PH_OPEN><<<(uint32_t)m, RWAVE, 0, k->st>>>(k->kc, d_open, d_rand, d_c, d_rho, m, sh.n_terms, d_terms, d_ev, d_u0, k->b_status.bytes(), 0);
            CG_KERNEL_CHECK();
            k->timer.mark(1, k->st);
            k_range_terms<<<ceil_div(m * sh.n_terms, RWAVE), RWAVE, 0, k->st>>>(k->d_shape.p + a.phase, k->d_tab_of[a.phase].p, d_terms, k->tab.p,
                                                                                 tab_slot, k->b_status.bytes(), m, k->b_part.p);
            CG_KERNEL_CHECK();
            k_range_sum<<<ceil_div(m * sh.n_pts, RWAVE), RWAVE, 0, k->st>>>(k->d_shape.p + a.phase, k->b_status.bytes(), m, k->b_part.p, d_u0,
                                                                           k->b_unc1.words_mut(), k->b_cmp.words_mut());
            CG_KERNEL_CHECK();
            k->timer.mark(2, k->st);
            k->b_unc0.down(k->st, a.unc0, off, m);
            k->b_unc1.down(k->st, a.unc1, off, m);
            k->b_cmp.down(k->st, a.cmp, off, m);
            k->b_evals.down(k->st, a.evals, off, m);
            k->b_status.down(k->st, a.status, off, m);
            CG_HIP(hipStreamSynchronize(k->st));
            k->timer.add();
        }
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}
}  // namespace

extern "C" int cg_range_commit_batch(cg_range_pk* k, uint32_t slot, const uint8_t* openings, const uint8_t* rand, uint64_t n,
                                     uint8_t* com_f, uint8_t* com_g, uint8_t* ts_out, uint8_t* status) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    return run_range(k, RpCall{PH_COMMIT, slot, openings, rand, nullptr, nullptr, n, com_f, com_g, ts_out, nullptr, status});
}

extern "C" int cg_range_quotient_batch(cg_range_pk* k, const uint8_t* openings, const uint8_t* rand, const uint8_t* c, uint64_t n,
                                       uint8_t* com_q, uint8_t* ts_q, uint8_t* status) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    return run_range(k, RpCall{PH_QUOTIENT, 0, openings, rand, c, nullptr, n, com_q, nullptr, ts_q, nullptr, status});
}

extern "C" int cg_range_open_batch(cg_range_pk* k, const uint8_t* openings, const uint8_t* rand, const uint8_t* c, const uint8_t* rho,
                                   uint64_t n, uint8_t* evals, uint8_t* proofs, uint8_t* status) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    return run_range(k, RpCall{PH_OPEN, 0, openings, rand, c, rho, n, proofs, nullptr, nullptr, evals, status});
}

// DLogPoK::prove's responses (dlog.rs:101-109) for the DLEQ of a range proof (rangeproof.rs:226-245): statement 0 holds
// (m, r) under the nonces (t_m, t_r), statement 1 (f0, f1, f2, m) under (t_f0, t_f1, t_f2, t_m).  Plain host arithmetic.
extern "C" int cg_range_respond_batch(const uint8_t* openings, const uint8_t* rand, const uint8_t* c_dleq, const uint8_t* status,
                                      uint64_t n, uint8_t* pok_s) {
    if (n == 0) return CG_OK;
    if (!openings || !rand || !c_dleq || !pok_s) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    static const int SECRET[RP_N_RESP] = {-1, -2, RP_F, RP_F + 1, RP_F + 2, -1};      // -1: m, -2: r, else a rand index
    static const int NONCE[RP_N_RESP] = {RP_TM, RP_TR, RP_TF, RP_TF + 1, RP_TF + 2, RP_TM};
    auto secret = [&](uint64_t p, uint32_t t) { return SECRET[t] < 0 ? openings + 64 * p + 32 * (-1 - SECRET[t]) : rand + 32 * (p * RP_N_RAND + SECRET[t]); };
    auto nonce = [&](uint64_t p, uint32_t t) { return rand + 32 * (p * RP_N_RAND + NONCE[t]); };
    return dlog_respond(n, RP_N_RESP, status, c_dleq, secret, nonce, pok_s, "an opening");
}

// `prove_n_bits` whole: the three phases above with the library's Merlin (merlin.hpp) between them.  Per chunk the inputs
// go up once, twelve kernels run back to back on the handle's stream - commit, the challenges c and c_dleq, quotient, the
// challenge rho, open, the responses - and the proof comes down once; the host waits once, for that copy.  The phases'
// kernels are the three calls' own, so the two paths give the same bytes.  The two stages are not timed apart here:
// cg_range_pk_last_kernel_ms reads zeros after this call.
//
// One body for the public call and for rangeproof.hpp's internal entry: rp_reserve, then per piece of at most RCHUNK
// showings rp_piece, which reads the openings and ped_com from device memory - the public call's own uploads, or what
// k_mk_shift of cg_create_showings_batch wrote - and waits for nothing.
namespace {
void rp_reserve(cg_range_pk* k, uint64_t chunk) {
    for (RowBuf* b : {&k->b_open, &k->b_rand, &k->b_c, &k->b_rho, &k->b_status, &k->o_ped, &k->o_pedc, &k->o_comf, &k->o_comg, &k->o_ts,
                      &k->o_comq, &k->o_tsq, &k->o_evals, &k->o_proofs, &k->o_pokc, &k->o_poks, &k->o_chal})
        b->reserve(chunk);
    const uint32_t max_terms = k->shape[PH_OPEN].n_terms;                  // the most of the three phases
    k->b_terms.reserve(chunk, 32 * max_terms);
    grow(k->b_part, chunk * max_terms);
    k->timer.reset();
}

void rp_piece(cg_range_pk* k, uint32_t slot, const uint32_t* d_open, const uint32_t* d_ped, const uint8_t* rand, uint64_t rand_pitch,
              const RangePkOut& out, uint64_t off, uint64_t m, uint8_t* d_status_out) {
    const G1Affine* tab_slot = k->slots.table(slot, "cg_range_pk_add_bases");
    const uint8_t* slot_cmp = k->slots.compressed(slot);
    if (rand_pitch == k->b_rand.row) k->b_rand.up(k->st, rand, 0, m);
    else CG_HIP(hipMemcpy2DAsync(k->b_rand.bytes(), k->b_rand.row, rand, rand_pitch, k->b_rand.row, m, hipMemcpyHostToDevice, k->st));
    const uint32_t* d_rand = k->b_rand.words();
    uint32_t *d_c = k->b_c.words_mut(), *d_rho = k->b_rho.words_mut(), *d_terms = k->b_terms.words_mut();
    uint32_t *d_ev = k->o_evals.words_mut(), *d_pr = k->o_proofs.words_mut();
    uint8_t* d_status = k->b_status.bytes();
    const uint32_t lanes = ceil_div(m, RWAVE);
    auto points = [&](int ph, uint32_t* unc0, uint32_t* unc1, uint32_t* cmp) {
        const RpShape& sh = k->shape[ph];
        k_range_terms<<<ceil_div(m * sh.n_terms, RWAVE), RWAVE, 0, k->st>>>(k->d_shape.p + ph, k->d_tab_of[ph].p, d_terms, k->tab.p, tab_slot,
                                                                             d_status, m, k->b_part.p);
        CG_KERNEL_CHECK();
        k_range_sum<<<ceil_div(m * sh.n_pts, RWAVE), RWAVE, 0, k->st>>>(k->d_shape.p + ph, d_status, m, k->b_part.p, unc0, unc1, cmp);
        CG_KERNEL_CHECK();
    };
    k_range_poly<PH_COMMIT><<<(uint32_t)m, RWAVE, 0, k->st>>>(k->kc, d_open, d_rand, d_c, d_rho, m, k->shape[PH_COMMIT].n_terms, d_terms, d_ev,
                                                              d_pr, d_status, 0);
    CG_KERNEL_CHECK();
    points(PH_COMMIT, k->o_comf.words_mut(), k->o_comg.words_mut(), k->o_ts.words_mut());
    k_range_challenge_c<<<lanes, RWAVE, 0, k->st>>>(k->o_ts.words(), d_ped, slot_cmp, k->key_cmp.p, d_status, m, k->o_pedc.words_mut(), d_c,
                                                   k->o_pokc.words_mut());
    CG_KERNEL_CHECK();
    k_range_poly<PH_QUOTIENT><<<(uint32_t)m, RWAVE, 0, k->st>>>(k->kc, d_open, d_rand, d_c, d_rho, m, k->shape[PH_QUOTIENT].n_terms, d_terms,
                                                                d_ev, d_pr, d_status, 1);
    CG_KERNEL_CHECK();
    points(PH_QUOTIENT, k->o_comq.words_mut(), nullptr, k->o_tsq.words_mut());
    k_range_challenge_rho<<<lanes, RWAVE, 0, k->st>>>(k->o_ts.words(), k->o_tsq.words(), d_status, m, d_rho);
    CG_KERNEL_CHECK();
    k_range_poly<PH_OPEN><<<(uint32_t)m, RWAVE, 0, k->st>>>(k->kc, d_open, d_rand, d_c, d_rho, m, k->shape[PH_OPEN].n_terms, d_terms, d_ev, d_pr,
                                                            d_status, 1);
    CG_KERNEL_CHECK();
    points(PH_OPEN, d_pr, nullptr, nullptr);
    const RpProof o{k->o_comf.words_mut(), k->o_comg.words_mut(), k->o_comq.words_mut(), d_ev, d_pr, k->o_pokc.words_mut(),
                    k->o_poks.words_mut(), k->o_chal.words_mut()};
    k_range_finish<<<lanes, RWAVE, 0, k->st>>>(d_open, d_rand, d_ped, d_c, d_rho, m, o, d_status);
    CG_KERNEL_CHECK();
    k->o_comf.down(k->st, out.com_f, off, m);
    k->o_comg.down(k->st, out.com_g, off, m);
    k->o_comq.down(k->st, out.com_q, off, m);
    k->o_evals.down(k->st, out.evals, off, m);
    k->o_proofs.down(k->st, out.proofs, off, m);
    k->o_pokc.down(k->st, out.pok_c, off, m);
    k->o_poks.down(k->st, out.pok_s, off, m);
    k->o_chal.down(k->st, out.challenges, off, m);
    k->b_status.down(k->st, out.status, off, m);
    if (d_status_out) CG_HIP(hipMemcpyAsync(d_status_out, d_status, m, hipMemcpyDeviceToDevice, k->st));
}
}  // namespace

extern "C" int cg_range_prove_batch(cg_range_pk* k, uint32_t slot, const uint8_t* openings, const uint8_t* ped_com, const uint8_t* rand,
                                    uint64_t n, uint8_t* com_f, uint8_t* com_g, uint8_t* com_q, uint8_t* evals, uint8_t* proofs,
                                    uint8_t* pok_c, uint8_t* pok_s, uint8_t* challenges_out, uint8_t* status) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    try {
        std::lock_guard<std::mutex> lk(k->mu);
        (void)k->slots.table(slot, "cg_range_pk_add_bases");
        if (n == 0) return CG_OK;
        if (!openings || !ped_com || !rand || !com_f || !com_g || !com_q || !evals || !proofs || !pok_c || !pok_s || !status)
            return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
        CG_HIP(hipSetDevice(k->device));
        const uint64_t chunk = n < RCHUNK ? n : RCHUNK;
        rp_reserve(k, chunk);
        const RangePkOut out{com_f, com_g, com_q, evals, proofs, pok_c, pok_s, challenges_out, status};
        for (uint64_t off = 0; off < n; off += chunk) {
            const uint64_t m = n - off < chunk ? n - off : chunk;
            k->b_open.up(k->st, openings, off, m);
            k->o_ped.up(k->st, ped_com, off, m);
            rp_piece(k, slot, k->b_open.words(), k->o_ped.words(), rand + off * k->b_rand.row, k->b_rand.row, out, off, m, nullptr);
            CG_HIP(hipStreamSynchronize(k->st));
        }
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}

namespace cg {
static_assert(RANGE_PK_PIECE == RCHUNK, "rangeproof.hpp states the piece of rangeproof.hip");
std::mutex& range_pk_lock(cg_range_pk* k) { return k->mu; }
int range_pk_device(const cg_range_pk* k) { return k->device; }
hipStream_t range_pk_stream(cg_range_pk* k) { return k->st; }
const uint8_t* range_pk_slot_bytes(const cg_range_pk* k, uint32_t slot) {
    return slot < k->slots.registered.size() ? k->slots.registered[slot].data() : nullptr;
}
void range_pk_reserve(cg_range_pk* k, uint64_t piece) { rp_reserve(k, piece < RCHUNK ? piece : RCHUNK); }
void range_pk_enqueue(cg_range_pk* k, uint32_t slot, const uint32_t* d_openings, const uint32_t* d_ped_com, const uint8_t* rand,
                      uint64_t rand_pitch, const RangePkOut& out, uint64_t off, uint64_t m, uint8_t* d_status) {
    rp_piece(k, slot, d_openings, d_ped_com, rand, rand_pitch, out, off, m, d_status);
}
}  // namespace cg
