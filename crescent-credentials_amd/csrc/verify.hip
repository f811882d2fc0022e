// Groth16 verification on the GPU: `Groth16::verify_with_processed_vk` (forks/groth16/src/verifier.rs:25-65) for a batch
// of proofs under one PreparedVerifyingKey, and `prepare_verifying_key` (verifier.rs:13-20) on the host, both over
// pairing.hpp.  What the reference's caller runs after every prove (creds/src/lib.rs:286-290).
//
// A cg_pvk holds one parsed key on a device: alpha_g1_beta_g2, the 91 line coefficients of gamma_g2_neg_pc and of
// delta_g2_neg_pc, gamma_abc_g1[0] and, for every other gamma_abc_g1 entry, a fixed-base table of 32 windows x 256
// multiples (8-bit windows: x_i·G_i is 32 mixed additions; fixed_base.hpp has the geometry, build_tables and the walk,
// fixed_base_mul, that every fixed-base lane below takes).  cg_verify_batch runs four kernels per chunk of proofs on the
// handle's own non-blocking stream:
//   k_vfy_inputs  one lane per (proof, input): x_i·gamma_abc[i+1] from the table                      -> XYZZ partials
//   k_vfy_check   one lane per proof: ark's checked deserialisation of A, B, C (coordinates < q, flags, curve, [r]B = O)
//                 and of the inputs (< r); gamma_abc[0] + Σ partials -> prepared inputs (affine)
//   k_vfy_miller  one lane per proof: the multi-Miller loop over (A, B on the fly), (prepared inputs, gamma), (C, delta)
//   k_vfy_final   one lane per proof: final exponentiation, == alpha_g1_beta_g2 -> one verdict byte
//
// cg_verify_show_batch verifies what a relying party receives instead: `ShowGroth16::verify` (creds/src/groth16rand.rs:232-306)
// for a batch of showings that share one io_types layout, up to the Merlin transcript, which stays with the host.  The key
// also carries a table of vk.delta_g1 (the last one), and a chunk of showings runs
//   k_show_terms  one lane per (showing, term): the fixed-base terms x_j·gamma_abc[j+1] of the revealed inputs and
//                 s·gamma_abc[i+1], s·delta_g1 of the DLogPoK responses from the tables; then, in waves of their own, the
//                 variable-base terms c·y_i by double-and-add                                          -> XYZZ partials
//   k_vfy_check   as above on the re-randomised proof, with no inputs
//   k_show_check  one lane per showing: checked deserialisation of com_hidden and the committed points, revealed inputs,
//                 responses and c < r; com_hidden + gamma_abc[0] + Σ committed + Σ revealed partials -> prepared inputs
//   k_show_k      one lane per (showing, statement): k_i = Σ_j s_ij·base_ij + c·y_i (creds/src/dlog.rs:137-145) from the
//                 partials, affine, written as ark-serialize's compressed G1 (what the transcript absorbs under b"k")
//   k_vfy_miller, k_vfy_final   unchanged
//
// cg_show_commit_batch creates such showings: `ClientState::show_groth16` (creds/src/groth16rand.rs:100-187) for a batch of
// client states that share one io_types layout, again up to the Merlin transcript, with every random scalar given by the
// caller.  The key also carries a table of the G1 generator (after delta_g1's) and one of vk.delta_g2 over Fq2, and a
// chunk of client states runs
//   k_mk_check    one lane per state: the proof's coordinates, flags and curve equations (no [r]B = O), read inputs and
//                 scalars < r, r1 and r2 non-zero                                                       -> one status byte
//   k_mk_fixed    one lane per (state, fixed-base term): secrets and nonces times gamma_abc[i+1] / delta_g1, and
//                 (Σ r_i + z)·G, from the tables                                                        -> XYZZ partials
//   k_mk_var      r1^-1·A and r2·A by double-and-add; in waves of their own r1·(B + r2·delta_g2) over Fq2   -> XYZZ partials
//   k_mk_out      one lane per (state, output point): A', B', C'' = C + r2·A - (Σ r_i + z)·G, com_hidden, the committed
//                 points and the k_i of DLogPoK::prove (creds/src/dlog.rs:60-75), affine, as ark-serialize writes them
// cg_show_respond_batch, the responses once the host's transcript has produced c, is host arithmetic.
//
// cg_verify_showings_batch verifies a showing whole: the cryptographic checks of `verify_show` (creds/src/lib.rs:630-658,
// :832-890) for a batch of showings of one layout, each with its range proofs.  It owns a cg_range_vk beside the cg_pvk and a
// chunk of showings runs, with nothing coming down in between,
//   k_show_link       one lane per (range, showing): ped_com = committed - t·gamma_abc[pos] (show_link.hpp) -> 64 B rows
//   the kernels of cg_verify_show_batch, unchanged
//   k_show_challenge  one lane per showing: the DLogPoK's Merlin transcript (merlin.hpp) over the compressed bases, the k_i of
//                     k_show_k and the y_i as their bytes stand; c' == pok_c keeps a showing accepted
//   the kernels of cg_range_verify_proofs_batch per range, on the range key's stream behind an event, reading ped_com where
//                     k_show_link wrote it (rangeverify.hpp's internal entry)
//   k_show_verdict    one lane per showing: the parts side by side and their conjunction
// cg_show_shift_batch is the creating side's link (lib.rs:370-372): k_show_shift, the same row routine with the opening.
//
// cg_create_showings_batch creates a showing whole: `create_show_proof` (creds/src/lib.rs:364-373, :468-471, :505-509) for a
// batch of client states of one layout, each with its range proofs.  It owns a cg_range_pk beside the cg_pvk and a chunk of
// client states runs, with nothing coming down in between,
//   k_mk_check, k_mk_fixed   as above
//   k_mk_out          the points that need the fixed-base partials alone: com_hidden, the committed points, the k_i
//   k_mk_shift        one lane per (range, showing): the link's opening (m - t, r) out of the showing's own inputs and rand
//                     (show_make.hpp) and ped_com = committed - t·gamma_abc[pos], where the range key's kernels read them
//   the kernels of cg_range_prove_batch per range and piece, on the range key's stream behind an event (rangeproof.hpp's
//                     internal entry), beside
//   k_mk_var, k_mk_out       the re-randomised proof
//   k_mk_challenge    one lane per showing: DLogPoK::prove's Merlin transcript (dlog.rs:56-99) over the compressed bases,
//                     the k_i and the y_i as k_mk_out wrote them -> c
//   k_mk_respond      one lane per (showing, response): s = nonce - c·secret (show_make.hpp, the row dlog_respond takes)
//   k_mk_parts        one lane per showing: the parts' status bytes side by side and their conjunction
//
// Shared by the three entries: the double-and-add chains are fixed_base.hpp's scalar_mul_254_mixed; ark_codec.hpp reads and
// writes every point on the device; io_layout parses a call's io_types once, for the verifier's and the creator's shapes
// alike; and the handle has one set of per-call arrays, named by what they hold.  Shared with the range keys, in
// key_handle.hpp: the handle's device, stream and lock, an array with its row width (RowBuf), the responses (dlog_respond).
#include <algorithm>
#include <memory>

#include "common.hpp"
#include "device_link.hpp"
#include "fixed_base.hpp"
#include "key_handle.hpp"
#include "pairing.hpp"
#include "pairing_team.hpp"
#include "rangeproof.hpp"
#include "rangeverify.hpp"
#include "show_link.hpp"
#include "show_make.hpp"

using namespace cg;

namespace {

constexpr uint64_t VCHUNK = 1u << 15;      // proofs per launch set
constexpr int VBLOCK = 64;
constexpr int NC = PairingConsts::N_COEFFS;

// one proof after k_vfy_check, Montgomery affine (identity = zeros)
struct alignas(16) ParsedProof {
    G1Affine a;
    G2Affine b;
    G1Affine c;
    G1Affine pi;     // prepared inputs
};
enum : uint8_t { ST_OK = 0, ST_MALFORMED = 2 };

struct HostVk {
    G1Affine alpha_g1, delta_g1;
    G2Affine beta_g2, gamma_g2, delta_g2;
    std::vector<G1Affine> gamma_abc;
};
static void read_vk(KeyRd& r, HostVk& vk) {       // data_structures.rs:31-44 (the fork's delta_g1 included)
    vk.alpha_g1 = r.g1();
    vk.beta_g2 = r.g2();
    vk.gamma_g2 = r.g2();
    vk.delta_g1 = r.g1();
    vk.delta_g2 = r.g2();
    const uint64_t n = r.count(64);
    vk.gamma_abc.resize(n);
    for (uint64_t i = 0; i < n; ++i) vk.gamma_abc[i] = r.g1();
}
// ark-ec bn::G2Prepared: ell_coeffs: Vec<(Fq2, Fq2, Fq2)>, infinity: bool
static bool read_g2_prepared(KeyRd& r, std::vector<EllCoeff>& c) {
    const uint64_t n = r.count(192);
    c.resize(n);
    for (uint64_t i = 0; i < n; ++i) {
        c[i].c0 = r.fq2();
        c[i].c1 = r.fq2();
        c[i].c2 = r.fq2();
    }
    r.need(1);
    const uint8_t inf = r.p[r.off++];
    if (inf > 1) throw HipError(CG_ERR_PARSE, "invalid bool in G2Prepared");
    if (!inf && n != (uint64_t)NC) throw HipError(CG_ERR_PARSE, "G2Prepared does not hold 91 line coefficients");
    return inf == 0;      // live
}

struct HostPvk {
    HostVk vk;
    Fq12 alpha_beta;
    std::vector<EllCoeff> gamma_c, delta_c;
    bool gamma_live = false, delta_live = false;
};
static void parse_pvk(const uint8_t* data, uint64_t len, HostPvk& k) {   // data_structures.rs:62-71
    KeyRd r{data, len, 0};
    read_vk(r, k.vk);
    Fq2* c[6] = {&k.alpha_beta.c0.c0, &k.alpha_beta.c0.c1, &k.alpha_beta.c0.c2,
                 &k.alpha_beta.c1.c0, &k.alpha_beta.c1.c1, &k.alpha_beta.c1.c2};
    for (int i = 0; i < 6; ++i) *c[i] = r.fq2();
    k.gamma_live = read_g2_prepared(r, k.gamma_c);
    k.delta_live = read_g2_prepared(r, k.delta_c);
    if (r.off != len) throw HipError(CG_ERR_PARSE, "trailing bytes after PreparedVerifyingKey");
}

__global__ __launch_bounds__(VBLOCK) void k_vfy_inputs(const uint32_t* __restrict__ inputs, uint64_t n, uint32_t ell,
                                                      const G1Affine* __restrict__ tab, G1XYZZ* __restrict__ part) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * ell) return;
    const uint32_t i = (uint32_t)(t % ell);
    const uint32_t* x = inputs + 8 * t;
    part[t] = fixed_base_mul(tab + (uint64_t)i * FB_NWIN * FB_WIN, x);
}

// SUBGROUP = false leaves [r]B = O to k_lone_subgroup (the latency arrangement)
template <bool SUBGROUP>
__global__ __launch_bounds__(VBLOCK) void k_vfy_check(const uint32_t* __restrict__ proofs, const uint32_t* __restrict__ inputs,
                                                     uint64_t n, uint32_t ell, const G1XYZZ* __restrict__ part, G1Affine g0,
                                                     ParsedProof* __restrict__ out, uint8_t* __restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t* w = proofs + 64 * p;
    bool ok = true;
    ParsedProof pp;
    pp.a = dev_g1(w, ok);
    pp.b = dev_g2<SUBGROUP>(w + 16, ok);
    pp.c = dev_g1(w + 48, ok);
    G1XYZZ acc = G1XYZZ::from_affine(g0);
    for (uint32_t i = 0; i < ell; ++i) {
        ok = ok && limbs_below(inputs + 8 * (p * ell + i), FrP::N);
        add(acc, part[p * ell + i]);
    }
    pp.pi = to_affine(acc);
    out[p] = pp;
    status[p] = ok ? ST_OK : ST_MALFORMED;
}

__global__ __launch_bounds__(VBLOCK) void k_vfy_miller(const ParsedProof* __restrict__ in, const uint8_t* __restrict__ status,
                                                      uint64_t n, const EllCoeff* gamma_c, const EllCoeff* delta_c,
                                                      int gamma_live, int delta_live, Fq12* __restrict__ f) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || status[p] != ST_OK) return;
    const ParsedProof pp = in[p];
    MillerPairs mp;
    mp.p[0] = pp.a; mp.q[0] = pp.b; mp.tab[0] = nullptr; mp.live[0] = !pp.a.is_inf() && !pp.b.is_inf();
    mp.p[1] = pp.pi; mp.q[1] = G2Affine::inf(); mp.tab[1] = gamma_c; mp.live[1] = !pp.pi.is_inf() && gamma_live;
    mp.p[2] = pp.c; mp.q[2] = G2Affine::inf(); mp.tab[2] = delta_c; mp.live[2] = !pp.c.is_inf() && delta_live;
    f[p] = multi_miller_loop<1>(mp);
}

__global__ __launch_bounds__(VBLOCK) void k_vfy_final(const Fq12* __restrict__ f, const uint8_t* __restrict__ status, uint64_t n,
                                                     Fq12 alpha_beta, uint8_t* __restrict__ verdict) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (status[p] != ST_OK) {
        verdict[p] = CG_VERIFY_MALFORMED;
        return;
    }
    Fq12 r;
    const bool some = final_exponentiation(f[p], r);
    verdict[p] = some && r == alpha_beta ? CG_VERIFY_ACCEPT : CG_VERIFY_REJECT;
}

// ---- the latency arrangement (cg_pvk_set_latency_mode): one workgroup per proof, pairing_team.hpp ------------------------
// the 254-step [r]B = O chain of k_vfy_check, on the handle's second stream beside the pairing, which does not need it:
// one lane per proof, B read as k_mk_check reads it.  A B that fails an earlier check is k_vfy_check<false>'s to report.
__global__ __launch_bounds__(VBLOCK) void k_lone_subgroup(const uint32_t* __restrict__ proofs, uint64_t n, uint8_t* __restrict__ in_g2) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    bool ok = true;
    const G2Affine b = dev_g2<false>(proofs + 64 * p + 16, ok);
    in_g2[p] = !ok || b.is_inf() || g2_in_subgroup(b);
}

__global__ __launch_bounds__(TEAM_WIDTH) void k_lone_miller(const ParsedProof* __restrict__ in, const uint8_t* __restrict__ status,
                                                          uint64_t n, const EllCoeff* gamma_c, const EllCoeff* delta_c,
                                                          int gamma_live, int delta_live, Fq12* __restrict__ f) {
    __shared__ TeamMem sh;
    const uint64_t p = blockIdx.x;
    // uniform: p is the workgroup's index and status[p] one byte that every lane of it reads
    if (p >= n || status[p] != ST_OK) return;
    const ParsedProof& pp = in[p];
    MillerPairs mp;
    mp.p[0] = pp.a; mp.q[0] = pp.b; mp.tab[0] = nullptr; mp.live[0] = !mp.p[0].is_inf() && !mp.q[0].is_inf();
    mp.p[1] = pp.pi; mp.q[1] = G2Affine::inf(); mp.tab[1] = gamma_c; mp.live[1] = !mp.p[1].is_inf() && gamma_live;
    mp.p[2] = pp.c; mp.q[2] = G2Affine::inf(); mp.tab[2] = delta_c; mp.live[2] = !mp.p[2].is_inf() && delta_live;
    team_miller_to<1>(sh, mp, f + p);
}

__global__ __launch_bounds__(TEAM_WIDTH) void k_lone_final(const Fq12* __restrict__ f, const uint8_t* __restrict__ status, uint64_t n,
                                                         Fq12 alpha_beta, uint8_t* __restrict__ verdict) {
    __shared__ TeamMem sh;
    const uint64_t p = blockIdx.x;
    if (p >= n) return;                          // uniform: the workgroup's index
    WaveLane ln{(int)threadIdx.x};
    if (status[p] != ST_OK) {                    // uniform: one byte that every lane of the workgroup reads
        if (ln.lane == 0) verdict[p] = CG_VERIFY_MALFORMED;
        return;
    }
    const bool some = team_final_of(sh, ln, f + p);
    const bool eq = some && team_equals(ln, sh, tp::reg(0), alpha_beta);
    if (ln.lane == 0) verdict[p] = eq ? CG_VERIFY_ACCEPT : CG_VERIFY_REJECT;
}

// after the two streams have met: a B outside the r-torsion makes the proof malformed, as k_vfy_check<true> would have
__global__ __launch_bounds__(VBLOCK) void k_lone_join(const uint8_t* __restrict__ in_g2, uint64_t n, uint8_t* __restrict__ status,
                                                     uint8_t* __restrict__ verdict) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || in_g2[p]) return;
    status[p] = ST_MALFORMED;
    verdict[p] = CG_VERIFY_MALFORMED;
}

// ---- showings (ShowGroth16::verify, groth16rand.rs:232-306) ------------------------------------------------------------
// One call's layout.  A showing's partials are [n_fixed fixed-base terms | n_var variable-base terms]: the revealed inputs,
// then (with a DLogPoK) the n_resp responses in the order dlog.rs:135-145 meets them, then c·y_i per statement.
struct ShowShape {
    uint32_t n_rev, n_com, n_resp;     // revealed inputs, committed inputs, responses = 2·n_com + n_hidden + 1
    uint32_t n_fixed, n_var;           // n_rev (+ n_resp), 0 or n_com + 1
    uint32_t n_terms;                  // n_fixed + n_var
};

__global__ __launch_bounds__(VBLOCK) void k_show_terms(const uint32_t* __restrict__ revealed, const uint32_t* __restrict__ pok_s,
                                                      const uint32_t* __restrict__ pok_c, const uint32_t* __restrict__ com_hidden,
                                                      const uint32_t* __restrict__ committed, uint64_t n, ShowShape sh,
                                                      const uint32_t* __restrict__ tab_of, const G1Affine* __restrict__ tab,
                                                      G1XYZZ* __restrict__ part) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_fixed_lanes = n * sh.n_fixed;
    if (g < n_fixed_lanes) {
        const uint64_t p = g / sh.n_fixed;
        const uint32_t t = (uint32_t)(g % sh.n_fixed);
        const uint32_t* x = t < sh.n_rev ? revealed + 8 * (p * sh.n_rev + t) : pok_s + 8 * (p * sh.n_resp + (t - sh.n_rev));
        part[p * sh.n_terms + t] = fixed_base_mul(tab + (uint64_t)tab_of[t] * FB_NWIN * FB_WIN, x);
        return;
    }
    // the variable-base lanes (a chain ~10x as long) start at a workgroup of their own
    const uint64_t var_at = (n_fixed_lanes + VBLOCK - 1) / VBLOCK * VBLOCK;
    if (g < var_at || g - var_at >= n * sh.n_var) return;
    const uint64_t v = g - var_at;
    const uint64_t p = v / sh.n_var;
    const uint32_t i = (uint32_t)(v % sh.n_var);
    const G1Affine y = dev_g1_unchecked(i < sh.n_com ? committed + 16 * (p * sh.n_com + i) : com_hidden + 16 * p);
    // c < r < 2^254 (a challenge is 248 bits, dlog.rs:97-99)
    part[p * sh.n_terms + sh.n_fixed + i] = scalar_mul_254_mixed(y, pok_c + 8 * p);
}

__global__ __launch_bounds__(VBLOCK) void k_show_check(const uint32_t* __restrict__ revealed, const uint32_t* __restrict__ pok_s,
                                                      const uint32_t* __restrict__ pok_c, const uint32_t* __restrict__ com_hidden,
                                                      const uint32_t* __restrict__ committed, uint64_t n, ShowShape sh,
                                                      const G1XYZZ* __restrict__ part, G1Affine g0, ParsedProof* __restrict__ out,
                                                      uint8_t* __restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    bool ok = true;
    G1XYZZ acc = G1XYZZ::from_affine(g0);                         // groth16rand.rs:246
    madd(acc, dev_g1(com_hidden + 16 * p, ok));
    for (uint32_t i = 0; i < sh.n_com; ++i) madd(acc, dev_g1(committed + 16 * (p * sh.n_com + i), ok));      // :269
    for (uint32_t j = 0; j < sh.n_rev; ++j) {                     // :279
        ok = ok && limbs_below(revealed + 8 * (p * sh.n_rev + j), FrP::N);
        add(acc, part[p * sh.n_terms + j]);
    }
    if (sh.n_var) {
        ok = ok && limbs_below(pok_c + 8 * p, FrP::N);
        for (uint32_t j = 0; j < sh.n_resp; ++j) ok = ok && limbs_below(pok_s + 8 * (p * sh.n_resp + j), FrP::N);
    }
    out[p].pi = to_affine(acc);
    if (!ok) status[p] = ST_MALFORMED;
}

__global__ __launch_bounds__(VBLOCK) void k_show_k(uint64_t n, ShowShape sh, const G1XYZZ* __restrict__ part,
                                                  const uint8_t* __restrict__ status, uint32_t* __restrict__ k_out) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * sh.n_var) return;
    const uint64_t p = g / sh.n_var;
    const uint32_t i = (uint32_t)(g % sh.n_var);
    uint32_t* out = k_out + 8 * g;
    if (status[p] != ST_OK) {
        for (int l = 0; l < 8; ++l) out[l] = 0;
        return;
    }
    // statement i < n_com: (gamma_abc[.], delta_g1); the last one: the hidden inputs' bases, then delta_g1
    const uint32_t lo = i < sh.n_com ? 2 * i : 2 * sh.n_com;
    const uint32_t hi = i < sh.n_com ? 2 * i + 2 : sh.n_resp;
    const G1XYZZ* pt = part + p * sh.n_terms;
    G1XYZZ acc = pt[sh.n_fixed + i];
    for (uint32_t j = lo; j < hi; ++j) add(acc, pt[sh.n_rev + j]);
    dev_put_g1(to_affine(acc), out, true);
}

// ---- whole showings (verify_show, creds/src/lib.rs:531-700): the challenge, the link, the conjunction --------------------
// The DLogPoK's transcript of a showing (dlog.rs:130-132, 147-169) and `c == self.c` (:171-174), one lane per showing, the
// sponge in LDS at ML_STATE bytes per lane as in k_rv_challenge*.  The bases come compressed, once per call, in the order
// the responses meet them (IoLayout::resp_tab); y_i is compressed here from committed / com_hidden as its bytes stand
// (y_cmp: n_com + 1 points of 8 words per showing); k_i is k_show_k's output, on the device already.  A showing whose status
// is not ST_OK has k_i of zero bytes and a verdict that says so: it is skipped.  c' goes out, with a byte c' == pok_c, and
// a showing stays CG_VERIFY_ACCEPT only where that byte is set.  Arithmetic on bytes only: no private segment.
// the transcript of showing p on either side of a showing: y_i compressed into y, then the challenge into c
__device__ __forceinline__ void show_transcript_lane(uint8_t* __restrict__ sponge_lane, const uint32_t* __restrict__ com_hidden,
                                                     const uint32_t* __restrict__ committed, uint64_t p, uint32_t n_com, uint32_t n_resp,
                                                     const uint8_t* __restrict__ bases_cmp, const uint32_t* __restrict__ k_pts,
                                                     const uint8_t* __restrict__ context, uint64_t context_len, uint32_t* __restrict__ y,
                                                     uint32_t* __restrict__ c) {
    const uint32_t n_stmt = n_com + 1, n_last = n_resp - 2 * n_com;
    for (uint32_t i = 0; i < n_com; ++i) ml_compress_g1(committed + 16 * (p * n_com + i), y + 8 * i);
    ml_compress_g1(com_hidden + 16 * p, y + 8 * n_com);
    ml_dlog_shape_challenge(sponge_lane, context, context_len, n_stmt, [=](uint32_t i) { return i < n_com ? 2u : n_last; }, bases_cmp,
                            (const uint8_t*)(k_pts + 8 * p * n_stmt), (const uint8_t*)y, (uint8_t*)c);
}
__global__ __launch_bounds__(VBLOCK) void k_show_challenge(const uint32_t* __restrict__ com_hidden, const uint32_t* __restrict__ committed,
                                                          const uint32_t* __restrict__ pok_c, uint64_t n, ShowShape sh,
                                                          const uint8_t* __restrict__ bases_cmp, const uint32_t* __restrict__ k_pts,
                                                          const uint8_t* __restrict__ context, uint64_t context_len, uint64_t context_stride,
                                                          const uint8_t* __restrict__ status, uint32_t* __restrict__ y_cmp,
                                                          uint32_t* __restrict__ c_out, uint8_t* __restrict__ same, uint8_t* __restrict__ verdict) {
    __shared__ __attribute__((aligned(8))) uint8_t sponge[VBLOCK * ML_STATE];
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    uint32_t* c = c_out + 8 * p;
    if (status[p] != ST_OK) {
        for (int l = 0; l < 8; ++l) c[l] = 0;
        same[p] = 0;
        return;
    }
    show_transcript_lane(sponge + ML_STATE * threadIdx.x, com_hidden, committed, p, sh.n_com, sh.n_resp, bases_cmp, k_pts,
                         context + p * context_stride, context_len, y_cmp + 8 * p * (sh.n_com + 1), c);
    uint32_t differ = 0;
    for (int l = 0; l < 8; ++l) differ |= c[l] ^ pok_c[8 * p + l];
    same[p] = differ == 0;
    if (differ && verdict[p] == CG_VERIFY_ACCEPT) verdict[p] = CG_VERIFY_REJECT;
}

// One row of the link (show_link.hpp): false where the commitment fails ark's checked deserialisation or the shift is >= r
__device__ __forceinline__ bool link_row(const uint32_t* __restrict__ commitment, const uint32_t* __restrict__ shift,
                                         const G1Affine* __restrict__ tab_of_input, G1Affine& ped_com) {
    bool ok = true;
    const G1Affine c = dev_g1(commitment, ok);
    ok = ok && link_below_r(shift);
    if (ok) ped_com = to_affine(shift_commitment(tab_of_input, c, shift));
    return ok;
}
// The verifying side: one lane per (range, showing), range-major so that a wave walks one table.  link: per range the
// committed index, then per range the table.  ped_com goes out as 64 B ark-uncompressed rows, range j's m rows at j·m, where
// the range key's kernels read them.  A malformed row is written with both flag bits set, which k_rv_check's checked
// deserialisation refuses as it refuses any such row: that range part is CG_VERIFY_MALFORMED.
__global__ __launch_bounds__(VBLOCK) void k_show_link(const uint32_t* __restrict__ committed, const uint32_t* __restrict__ shifts, uint64_t n,
                                                     uint32_t n_com, uint32_t n_ranges, const uint32_t* __restrict__ link,
                                                     const G1Affine* __restrict__ tab, uint32_t* __restrict__ ped_com) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * n_ranges) return;
    const uint32_t j = (uint32_t)(g / n);
    const uint64_t p = g % n;
    uint32_t* out = ped_com + 16 * g;
    G1Affine pc;
    if (link_row(committed + 16 * (p * n_com + link[j]), shifts + 8 * (p * n_ranges + j), tab + (uint64_t)link[n_ranges + j] * FB_NWIN * FB_WIN, pc))
        dev_put_g1(pc, out, false);
    else
        for (int l = 0; l < 16; ++l) out[l] = 0xFFFFFFFFu;
}
// The creating side (cg_show_shift_batch): one lane per opening of one input; m' = m - t, r as it is, c' = c - t·base
__global__ __launch_bounds__(VBLOCK) void k_show_shift(const uint32_t* __restrict__ openings, const uint32_t* __restrict__ commitments,
                                                      const uint32_t* __restrict__ shifts, uint64_t n, const G1Affine* __restrict__ tab_of_input,
                                                      uint32_t* __restrict__ openings_out, uint32_t* __restrict__ ped_com, uint8_t* __restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t *op = openings + 16 * p, *t = shifts + 8 * p;
    G1Affine pc;
    const bool ok = link_below_r(op) && link_below_r(op + 8) && link_row(commitments + 16 * p, t, tab_of_input, pc);
    status[p] = ok ? CG_SHOW_MADE : CG_SHOW_MALFORMED;
    if (!ok) {
        for (int l = 0; l < 16; ++l) openings_out[16 * p + l] = ped_com[16 * p + l] = 0;
        return;
    }
    shift_opening(op, t, openings_out + 16 * p);
    for (int l = 0; l < 8; ++l) openings_out[16 * p + 8 + l] = op[8 + l];
    dev_put_g1(pc, ped_com + 16 * p, false);
}

// The conjunction, one lane per showing: the Groth16 part, then the range parts (range j's m bytes at j·m) -> parts, row per
// showing, and the showing's verdict: MALFORMED if any part is, ACCEPT if every part is, else REJECT
__global__ __launch_bounds__(VBLOCK) void k_show_verdict(const uint8_t* __restrict__ groth, const uint8_t* __restrict__ range, uint64_t n,
                                                        uint32_t n_ranges, uint8_t* __restrict__ parts, uint8_t* __restrict__ verdict) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    bool malformed = false, accept = true;
    for (uint32_t j = 0; j <= n_ranges; ++j) {
        const uint8_t v = j ? range[(j - 1) * n + p] : groth[p];
        parts[p * (n_ranges + 1) + j] = v;
        malformed = malformed || v == CG_VERIFY_MALFORMED;
        accept = accept && v == CG_VERIFY_ACCEPT;
    }
    verdict[p] = malformed ? CG_VERIFY_MALFORMED : accept ? CG_VERIFY_ACCEPT : CG_VERIFY_REJECT;
}

// ---- creating showings (ClientState::show_groth16, groth16rand.rs:100-187) ---------------------------------------------
// One call's layout.  A showing's G1 partials are [n_fix fixed-base terms | r1^-1·A | r2·A]; the fixed-base terms are the
// n_resp secrets times their bases in the order dlog.rs:60-67 meets them (x_i·gamma_abc[i+1], r_i·delta_g1 per committed
// input, x_j·gamma_abc[j+1] per hidden input, z·delta_g1), then the n_resp nonces times the same bases, then
// (Σ r_i + z)·G.  `desc` on the device is [table of term t | scalar of term t]: an index into the showing's inputs, or with
// MK_RAND set into its rand.
struct MkShape {
    uint32_t n_io, n_com, n_resp, n_rand;     // n_rand = 3 + n_com + n_resp: r1, r2, the r_i, z, the nonces
    uint32_t n_fix;                           // 2·n_resp + 1
    uint32_t n_terms;                         // n_fix + 2
    uint32_t n_out;                           // points written per showing: A', B', C'', com_hidden, n_com committed, n_com + 1 k
};
constexpr uint32_t MK_RAND = 0x80000000u;

__global__ __launch_bounds__(VBLOCK) void k_mk_fixed(const uint32_t* __restrict__ inputs, const uint32_t* __restrict__ rand, uint64_t n,
                                                    MkShape sh, const uint32_t* __restrict__ desc, const G1Affine* __restrict__ tab,
                                                    G1XYZZ* __restrict__ part) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * sh.n_fix) return;
    const uint64_t p = g / sh.n_fix;
    const uint32_t t = (uint32_t)(g % sh.n_fix);
    const uint32_t* rd = rand + 8 * p * sh.n_rand;
    Fr x;
    if (t + 1 == sh.n_fix) {                                      // acc_r + z (groth16rand.rs:136, :167), mod r
        x = dev_fr(rd + 8 * 2);
        for (uint32_t j = 1; j <= sh.n_com; ++j) x = add(x, dev_fr(rd + 8 * (2 + j)));
    } else {
        const uint32_t src = desc[sh.n_fix + t];
        x = dev_fr(src & MK_RAND ? rd + 8 * (src & ~MK_RAND) : inputs + 8 * (p * sh.n_io + src));
    }
    part[p * sh.n_terms + t] = fixed_base_mul(tab + (uint64_t)desc[t] * FB_NWIN * FB_WIN, x.l);
}

// the chains of rerandomize_proof (prover.rs:239-253): lanes [0, n) r1^-1·A, lanes [n, 2n) r2·A, and from a workgroup of
// their own the G2 lanes r1·(B + r2·delta_g2), one multiplication over Fq2 each and several times as long.  Nothing is
// checked here: k_mk_check does that, and k_mk_out writes zeros for a showing that fails.
__global__ __launch_bounds__(VBLOCK) void k_mk_var(const uint32_t* __restrict__ proofs, const uint32_t* __restrict__ rand, uint64_t n,
                                                  MkShape sh, const G2Affine* __restrict__ tab_g2, G1XYZZ* __restrict__ part,
                                                  G2XYZZ* __restrict__ part_g2) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < 2 * n) {
        const uint32_t which = g >= n;
        const uint64_t p = g - which * n;
        const G1Affine a = dev_g1_unchecked(proofs + 64 * p);
        Fr k = dev_fr(rand + 8 * (p * sh.n_rand + which));
        if (!which) k = from_mont(inv(to_mont(k)));               // r1 = 0 stays 0; that showing is malformed
        part[p * sh.n_terms + sh.n_fix + which] = scalar_mul_254_mixed(a, k.l);
        return;
    }
    const uint64_t g2_at = (2 * n + VBLOCK - 1) / VBLOCK * VBLOCK;
    if (g < g2_at || g - g2_at >= n) return;
    const uint64_t p = g - g2_at;
    G2XYZZ acc = fixed_base_mul(tab_g2, rand + 8 * (p * sh.n_rand + 1));         // r2·delta_g2
    madd(acc, dev_g2_unchecked(proofs + 64 * p + 16));
    part_g2[p] = scalar_mul_254_mixed(to_affine(acc), rand + 8 * p * sh.n_rand);
}

// one lane per showing: the checks of dev_g1 / dev_g2 on the proof without [r]B = O (a client state is the host's own
// data, which the reference reads unchecked), every read input and every rand scalar < r, r1 and r2 non-zero
__global__ __launch_bounds__(VBLOCK) void k_mk_check(const uint32_t* __restrict__ proofs, const uint32_t* __restrict__ inputs,
                                                    const uint32_t* __restrict__ rand, uint64_t n, MkShape sh,
                                                    const uint32_t* __restrict__ desc, uint8_t* __restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t* w = proofs + 64 * p;
    bool ok = true;
    (void)dev_g1(w, ok);
    (void)dev_g2<false>(w + 16, ok);
    (void)dev_g1(w + 48, ok);
    for (uint32_t t = 0; t < sh.n_resp; ++t) {
        const uint32_t src = desc[sh.n_fix + t];
        if (!(src & MK_RAND)) ok = ok && limbs_below(inputs + 8 * (p * sh.n_io + src), FrP::N);
    }
    const uint32_t* rd = rand + 8 * p * sh.n_rand;
    for (uint32_t j = 0; j < sh.n_rand; ++j) ok = ok && limbs_below(rd + 8 * j, FrP::N);
    ok = ok && !dev_fr(rd).is_zero() && !dev_fr(rd + 8).is_zero();          // the reference redraws these (prover.rs:234-237)
    status[p] = ok ? CG_SHOW_MADE : CG_SHOW_MALFORMED;
}

// one lane per (showing, output point): the partials summed with the general `add` (two of them coincide or cancel for
// chosen randomness), affine, written as ark-serialize writes them; zeros for a malformed showing.  A launch writes the
// points [o_lo, o_lo + o_n) of every showing: all n_out of them, or - cg_create_showings_batch - the points from 3 on, which
// need k_mk_fixed's partials alone, before k_mk_var and A', B', C'' behind it
__global__ __launch_bounds__(VBLOCK) void k_mk_out(const uint32_t* __restrict__ proofs, uint64_t n, MkShape sh, uint32_t o_lo, uint32_t o_n,
                                                  const G1XYZZ* __restrict__ part, const G2XYZZ* __restrict__ part_g2,
                                                  const uint8_t* __restrict__ status, uint32_t* __restrict__ rand_proofs,
                                                  uint32_t* __restrict__ com_hidden, uint32_t* __restrict__ committed,
                                                  uint32_t* __restrict__ k_out) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * o_n) return;
    const uint64_t p = g / o_n;
    const uint32_t o = o_lo + (uint32_t)(g % o_n);
    const bool made = status[p] == CG_SHOW_MADE;
    const G1XYZZ* pt = part + p * sh.n_terms;
    if (o == 1) {                                                 // B' = r1·(B + r2·delta_g2)
        uint32_t* out = rand_proofs + 64 * p + 16;
        if (made) dev_put_g2(to_affine(part_g2[p]), out);
        else for (int l = 0; l < 32; ++l) out[l] = 0;
        return;
    }
    uint32_t* out;
    uint32_t lo, hi;                                              // the fixed-base partials [lo, hi) of this point
    bool compressed = false;
    G1XYZZ acc = G1XYZZ::inf();
    if (o == 0) {                                                 // A' = r1^-1·A
        out = rand_proofs + 64 * p;
        lo = hi = 0;
        acc = pt[sh.n_fix];
    } else if (o == 2) {                                          // C'' = C + r2·A - (acc_r + z)·G
        out = rand_proofs + 64 * p + 48;
        lo = hi = 0;
        if (made) {
            acc = G1XYZZ::from_affine(dev_g1_unchecked(proofs + 64 * p + 48));
            add(acc, pt[sh.n_fix + 1]);
            add(acc, neg(pt[sh.n_fix - 1]));
        }
    } else if (o == 3) {                                          // Σ x_j·gamma_abc[j+1] + z·delta_g1 over the hidden inputs
        out = com_hidden + 16 * p;
        lo = 2 * sh.n_com, hi = sh.n_resp;
    } else if (o < 4 + sh.n_com) {                                // x_i·gamma_abc[i+1] + r_i·delta_g1
        const uint32_t i = o - 4;
        out = committed + 16 * (p * sh.n_com + i);
        lo = 2 * i, hi = 2 * i + 2;
    } else {                                                      // k_i = Σ_j rho_ij·base_ij (dlog.rs:60-67)
        const uint32_t i = o - 4 - sh.n_com;
        out = k_out + 8 * (p * (sh.n_com + 1) + i);
        compressed = true;
        lo = sh.n_resp + (i < sh.n_com ? 2 * i : 2 * sh.n_com);
        hi = i < sh.n_com ? lo + 2 : 2 * sh.n_resp;
    }
    if (!made) {
        for (int l = 0; l < (compressed ? 8 : 16); ++l) out[l] = 0;
        return;
    }
    for (uint32_t j = lo; j < hi; ++j) add(acc, pt[j]);
    dev_put_g1(to_affine(acc), out, compressed);
}

// ---- creating whole showings (create_show_proof, creds/src/lib.rs:364-373, :468-471, :505-509) ----------------------------
// DLogPoK::prove's transcript (dlog.rs:56-99), one lane per showing, the sponge in LDS at ML_STATE bytes per lane as in
// k_show_challenge, whose text it shares (show_transcript_lane): the bases compressed once per call in resp_tab order, y_i
// compressed here from committed / com_hidden and k_i read as k_mk_out wrote them.  A showing that is not CG_SHOW_MADE has
// zero rows there and gets c = 0.  Arithmetic on bytes only: no private segment.
__global__ __launch_bounds__(VBLOCK) void k_mk_challenge(const uint32_t* __restrict__ com_hidden, const uint32_t* __restrict__ committed, uint64_t n,
                                                        MkShape sh, const uint8_t* __restrict__ bases_cmp, const uint32_t* __restrict__ k_pts,
                                                        const uint8_t* __restrict__ context, uint64_t context_len, uint64_t context_stride,
                                                        const uint8_t* __restrict__ status, uint32_t* __restrict__ y_cmp, uint32_t* __restrict__ c_out) {
    __shared__ __attribute__((aligned(8))) uint8_t sponge[VBLOCK * ML_STATE];
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    uint32_t* c = c_out + 8 * p;
    if (status[p] != CG_SHOW_MADE) {
        for (int l = 0; l < 8; ++l) c[l] = 0;
        return;
    }
    show_transcript_lane(sponge + ML_STATE * threadIdx.x, com_hidden, committed, p, sh.n_com, sh.n_resp, bases_cmp, k_pts,
                         context + p * context_stride, context_len, y_cmp + 8 * p * (sh.n_com + 1), c);
}

// DLogPoK::prove's responses (dlog.rs:101-109), one lane per (showing, response): the secret and the nonce where `desc`
// says k_mk_fixed read them, c to Montgomery form once per lane (k_range_finish does it once per showing, for six rows),
// then show_make.hpp's row.  k_mk_check found every scalar below r; zeros for a showing it refused.
__global__ __launch_bounds__(VBLOCK) void k_mk_respond(const uint32_t* __restrict__ inputs, const uint32_t* __restrict__ rand,
                                                      const uint32_t* __restrict__ c, uint64_t n, MkShape sh, const uint32_t* __restrict__ desc,
                                                      const uint8_t* __restrict__ status, uint32_t* __restrict__ pok_s) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * sh.n_resp) return;
    const uint64_t p = g / sh.n_resp;
    const uint32_t t = (uint32_t)(g % sh.n_resp);
    uint32_t* s = pok_s + 8 * g;
    if (status[p] != CG_SHOW_MADE) {
        for (int l = 0; l < 8; ++l) s[l] = 0;
        return;
    }
    const uint32_t src = desc[sh.n_fix + t], nonce = desc[sh.n_fix + sh.n_resp + t] & ~MK_RAND;
    const uint32_t* rd = rand + 8 * p * sh.n_rand;
    mk_response_row(mk_challenge_mont(c + 8 * p), src & MK_RAND ? rd + 8 * (src & ~MK_RAND) : inputs + 8 * (p * sh.n_io + src), rd + 8 * nonce, s);
}

// The creating side's link inside the call: one lane per (range, showing), range-major so that a wave walks one table, as
// k_show_link.  link: per range the committed index, then per range the input (its table).  The opening is the showing's
// own (show_make.hpp): m = inputs[pos], r = r_ci of rand; the row is k_show_shift's - m, r, t below r, the committed point as
// k_mk_out wrote it through the checked read - and it goes out as (m - t, r), 64 B, and ped_com, 64 B, range j's m rows at
// j·m, where the range key's kernels read them, with a made byte per row.
// How the range half learns of a refused row (the showing is not CG_SHOW_MADE, or a scalar is >= r): its opening is written
// as zeros and its ped_com with both flag bits set.  k_range_finish's checked read of ped_com refuses that as it refuses
// any such row, zeroes every output row of the proof and sets its status to CG_SHOW_MALFORMED; k_mk_parts also reads the
// made byte.
__global__ __launch_bounds__(VBLOCK) void k_mk_shift(const uint32_t* __restrict__ inputs, const uint32_t* __restrict__ rand,
                                                    const uint32_t* __restrict__ committed, const uint32_t* __restrict__ shifts,
                                                    const uint8_t* __restrict__ status, uint64_t n, MkShape sh, uint32_t n_ranges,
                                                    const uint32_t* __restrict__ link, const G1Affine* __restrict__ tab,
                                                    uint32_t* __restrict__ openings, uint32_t* __restrict__ ped_com, uint8_t* __restrict__ made) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * n_ranges) return;
    const uint32_t j = (uint32_t)(g / n);
    const uint64_t p = g % n;
    const uint32_t ci = link[j], pos = link[n_ranges + j];
    const MkOpeningAt at = mk_link_opening(p, sh.n_io, sh.n_rand, pos, ci);
    const uint32_t *m = inputs + 8 * at.m, *r = rand + 8 * at.r, *t = shifts + 8 * (p * n_ranges + j);
    uint32_t *op = openings + 16 * g, *pc_out = ped_com + 16 * g;
    G1Affine pc;
    const bool ok = status[p] == CG_SHOW_MADE && link_below_r(m) && link_below_r(r) &&
                    link_row(committed + 16 * (p * sh.n_com + ci), t, tab + (uint64_t)pos * FB_NWIN * FB_WIN, pc);
    made[g] = ok ? CG_SHOW_MADE : CG_SHOW_MALFORMED;
    if (!ok) {
        for (int l = 0; l < 16; ++l) {
            op[l] = 0;
            pc_out[l] = 0xFFFFFFFFu;
        }
        return;
    }
    shift_opening(m, t, op);
    for (int l = 0; l < 8; ++l) op[8 + l] = r[l];
    dev_put_g1(pc, pc_out, false);
}

// The conjunction, one lane per showing: the Groth16 part, then the range parts (range j's m bytes at j·m: made only where
// k_mk_shift made the row and the range key's kernels the proof) -> parts, row per showing, and the showing's status
__global__ __launch_bounds__(VBLOCK) void k_mk_parts(const uint8_t* __restrict__ groth, const uint8_t* __restrict__ shift_made,
                                                    const uint8_t* __restrict__ range, uint64_t n, uint32_t n_ranges,
                                                    uint8_t* __restrict__ parts, uint8_t* __restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    bool all = groth[p] == CG_SHOW_MADE;
    parts[p * (n_ranges + 1)] = groth[p];
    for (uint32_t j = 0; j < n_ranges; ++j) {
        const bool made = shift_made[j * n + p] == CG_SHOW_MADE && range[j * n + p] == CG_SHOW_MADE;
        parts[p * (n_ranges + 1) + 1 + j] = made ? CG_SHOW_MADE : CG_SHOW_MALFORMED;
        all = all && made;
    }
    status[p] = all ? CG_SHOW_MADE : CG_SHOW_MALFORMED;
}

}  // namespace

struct cg_pvk : KeyHandle {
    uint64_t n_inputs = 0;
    G1Affine g0;
    Fq12 alpha_beta;
    int gamma_live = 0, delta_live = 0;
    bool gamma_is_one = false;             // gamma_g2 is the G2 generator: what cg_show_commit_batch's correction of C assumes
    DevBuf<G1Affine> tab;                  // gamma_abc_g1[1..], delta_g1, the G1 generator
    DevBuf<G2Affine> tab_g2;               // delta_g2
    DevBuf<EllCoeff> gamma_c, delta_c;
    // per-call arrays, named by what they hold and shared by the three entries: each is grown, never shrunk, to the largest
    // chunk and layout seen.  Bytes are ark-serialize's, as the caller passes and receives them; a width that depends on the
    // call's io_types is set by the call.
    RowBuf b_proofs{256};                  // proofs in
    RowBuf b_inputs;                       // scalars per (item, input): public inputs, revealed inputs, a client state's inputs
    RowBuf b_rows;                         // scalars per (item, row): the responses of a showing, or a client state's rand
    RowBuf b_chal{32};                     // the challenge c per item
    RowBuf b_comh{64}, b_comm, b_k;        // com_hidden, the committed points and the k points per item, read or written
    RowBuf b_rproofs{256};                 // re-randomised proofs out
    RowBuf b_status{1}, b_verdict{1};
    DevBuf<G1XYZZ> b_part;
    DevBuf<G2XYZZ> b_part_g2;
    DevBuf<ParsedProof> b_parsed;
    DevBuf<Fq12> b_miller;
    DevBuf<uint32_t> b_desc;               // the call's term descriptor: tab_of of k_show_terms, desc of k_mk_*
    // the two arrangements of the pairing stage (cg_pvk_set_latency_mode); the latency one also runs [r]B = O on a second stream
    bool latency = false;
    StageTimer timer;                      // the group stage, the pairing
    hipStream_t st2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    RowBuf b_in_g2{1};
    // whole showings (cg_verify_showings_batch, cg_show_shift_batch).  On the host the 64 bytes of gamma_abc_g1[1..] and of
    // delta_g1 (the last one) as the key holds them: what a range key's slot must have registered, and what the DLogPoK's
    // transcript absorbs once compressed.  On the device per call the compressed bases and the contexts, per showing the
    // compressed y_i, c' and the byte c' == pok_c, per (showing, range) the shift and ped_com - read there by the range
    // key's kernels, whose verdicts come back into b_rverd -, then the parts and the verdict.
    std::vector<uint8_t> base_bytes;
    bool overlap = true;                   // cg_pvk_set_showings_overlap
    DevBuf<uint8_t> b_bases_cmp;
    RowBuf b_ctx, b_ycmp, b_cprime{32}, b_same{1}, b_shift, b_link, b_rverd, b_parts, b_final{1};
    hipEvent_t ev_link = nullptr, ev_ranges = nullptr;      // the range key's stream behind the link, ours behind its last kernel
    // creating whole showings (cg_create_showings_batch) also: the responses, and per (showing, range) the link's opening and
    // made byte; ped_com is in b_link and the range parts' status bytes come back into b_rverd
    RowBuf b_resp, b_lopen, b_lmade;
    // the device link (cg_device_link_verify_batch, devicelink.hip): its per-call arrays, which that file creates and names
    void* dl_state = nullptr;
    void (*dl_free)(void*) = nullptr;
    // and those of cg_device_link_prove_batch (devicelinkmake.hip)
    void* dlm_state = nullptr;
    void (*dlm_free)(void*) = nullptr;
    // and the Poseidon constants and arrays of the h_Q entries (devicelinkmake.hip)
    void* hq_state = nullptr;
    void (*hq_free)(void*) = nullptr;
    // and the table of P-256's generator and the arrays of the P-256 entries (p256tu.hip)
    void* p256_state = nullptr;
    void (*p256_free)(void*) = nullptr;
    void open_second() {
        CG_HIP(hipStreamCreateWithFlags(&st2, hipStreamNonBlocking));
        for (hipEvent_t* e : {&ev_fork, &ev_join, &ev_link, &ev_ranges}) CG_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    ~cg_pvk() {                            // both streams are waited for before the buffers above are freed (key_handle.hpp)
        if (st2) { (void)hipStreamSynchronize(st2); (void)hipStreamDestroy(st2); }
        drain();
        if (dl_state) dl_free(dl_state);
        if (dlm_state) dlm_free(dlm_state);
        if (hq_state) hq_free(hq_state);
        if (p256_state) p256_free(p256_state);
        for (hipEvent_t e : {ev_fork, ev_join, ev_link, ev_ranges}) if (e) (void)hipEventDestroy(e);
    }

    // the stages both verifying entries share, on a chunk of m proofs already in b_proofs; all under the handle's lock
    // right after the proofs' copy: in the latency arrangement the subgroup chain starts on the second stream
    void proofs_up(const uint8_t* proofs, uint64_t off, uint64_t m) {
        b_proofs.up(st, proofs, off, m);
        if (!latency) return;
        CG_HIP(hipEventRecord(ev_fork, st));
        CG_HIP(hipStreamWaitEvent(st2, ev_fork, 0));
        k_lone_subgroup<<<ceil_div(m, VBLOCK), VBLOCK, 0, st2>>>(b_proofs.words(), m, b_in_g2.bytes());
        CG_KERNEL_CHECK();
        CG_HIP(hipEventRecord(ev_join, st2));
    }
    void check(uint64_t m, const uint32_t* d_inputs, uint32_t ell) {
        const uint32_t grid = ceil_div(m, VBLOCK);
        if (latency) k_vfy_check<false><<<grid, VBLOCK, 0, st>>>(b_proofs.words(), d_inputs, m, ell, b_part.p, g0, b_parsed.p, b_status.bytes());
        else k_vfy_check<true><<<grid, VBLOCK, 0, st>>>(b_proofs.words(), d_inputs, m, ell, b_part.p, g0, b_parsed.p, b_status.bytes());
        CG_KERNEL_CHECK();
    }
    // Miller loop and final exponentiation; in the latency arrangement then the meeting with the second stream, after
    // which status and verdict are what the wide arrangement writes
    void pairing(uint64_t m) {
        if (latency) {
            k_lone_miller<<<(uint32_t)m, TEAM_WIDTH, 0, st>>>(b_parsed.p, b_status.bytes(), m, gamma_c.p, delta_c.p, gamma_live, delta_live, b_miller.p);
            CG_KERNEL_CHECK();
            k_lone_final<<<(uint32_t)m, TEAM_WIDTH, 0, st>>>(b_miller.p, b_status.bytes(), m, alpha_beta, b_verdict.bytes());
            CG_KERNEL_CHECK();
            CG_HIP(hipStreamWaitEvent(st, ev_join, 0));
            k_lone_join<<<ceil_div(m, VBLOCK), VBLOCK, 0, st>>>(b_in_g2.bytes(), m, b_status.bytes(), b_verdict.bytes());
            CG_KERNEL_CHECK();
            return;
        }
        const uint32_t grid = ceil_div(m, VBLOCK);
        k_vfy_miller<<<grid, VBLOCK, 0, st>>>(b_parsed.p, b_status.bytes(), m, gamma_c.p, delta_c.p, gamma_live, delta_live, b_miller.p);
        CG_KERNEL_CHECK();
        k_vfy_final<<<grid, VBLOCK, 0, st>>>(b_miller.p, b_status.bytes(), m, alpha_beta, b_verdict.bytes());
        CG_KERNEL_CHECK();
    }
};

extern "C" int cg_pvk_load(cg_pvk** out, const uint8_t* pvk_bytes, uint64_t len, int32_t device) {
    if (!out || !pvk_bytes) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    try {
        HostPvk hk;
        parse_pvk(pvk_bytes, len, hk);           // host only: a parse error is reported before any HIP call
        if (hk.vk.gamma_abc.empty()) return fail(CG_ERR_MALFORMED_KEY, "gamma_abc_g1 is empty");
        // the tables: build_tables skips gamma_abc[0], so table i is gamma_abc[i+1]'s, table n_inputs delta_g1's and table
        // n_inputs + 1 the generator's
        std::vector<G1Affine> bases = hk.vk.gamma_abc, tab;
        bases.push_back(hk.vk.delta_g1);            // the Pedersen / DLogPoK base of a showing (groth16rand.rs:133, :274)
        bases.push_back(g1_generator());            // G: the correction of C in a showing (groth16rand.rs:167)
        build_tables(bases, tab);
        std::vector<G2Affine> tab_g2;                   // r2·delta_g2 of rerandomize_proof (prover.rs:247)
        build_tables(std::vector<G2Affine>{G2Affine::inf(), hk.vk.delta_g2}, tab_g2);
        const G2Affine g2_gen = g2_generator();
        std::unique_ptr<cg_pvk> k(new cg_pvk());
        k->n_inputs = hk.vk.gamma_abc.size() - 1;
        k->g0 = hk.vk.gamma_abc[0];
        k->alpha_beta = hk.alpha_beta;
        k->gamma_live = hk.gamma_live;
        k->delta_live = hk.delta_live;
        k->gamma_is_one = hk.vk.gamma_g2.x == g2_gen.x && hk.vk.gamma_g2.y == g2_gen.y;       // generator.rs:28
        // the key starts with its VerifyingKey: alpha_g1 64 | beta_g2 128 | gamma_g2 128 | delta_g1 64 | delta_g2 128 | u64 | gamma_abc_g1
        k->base_bytes.assign(pvk_bytes + 520 + 64, pvk_bytes + 520 + 64 * hk.vk.gamma_abc.size());
        k->base_bytes.insert(k->base_bytes.end(), pvk_bytes + 320, pvk_bytes + 384);
        k->open(device);
        k->open_second();
        k->timer.create();
        k->tab.alloc(tab.size() ? tab.size() : 1);
        h2d_sync(k->tab.p, tab.data(), tab.size() * sizeof(G1Affine), k->st);
        k->tab_g2.alloc(tab_g2.size());
        h2d_sync(k->tab_g2.p, tab_g2.data(), tab_g2.size() * sizeof(G2Affine), k->st);
        k->gamma_c.alloc(NC);
        k->delta_c.alloc(NC);
        if (hk.gamma_live) h2d_sync(k->gamma_c.p, hk.gamma_c.data(), NC * sizeof(EllCoeff), k->st);
        if (hk.delta_live) h2d_sync(k->delta_c.p, hk.delta_c.data(), NC * sizeof(EllCoeff), k->st);
        *out = k.release();
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}

extern "C" int cg_pvk_num_inputs(const cg_pvk* k, uint64_t* n) {
    if (!k || !n) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    *n = k->n_inputs;
    return CG_OK;
}

extern "C" int cg_pvk_set_latency_mode(cg_pvk* k, int32_t on) { return set_latency_mode(k, on); }

// Diagnostic: what the kernels of the handle's last verifying call took, by HIP events, summed over its chunks: the group
// stage (tables, checks, sums) and the pairing (Miller loop and final exponentiation; in the latency arrangement with
// the wait for the subgroup chain, and for a showing with k_show_k, which follows it there)
extern "C" int cg_pvk_last_kernel_ms(cg_pvk* k, float* group_ms, float* pairing_ms) { return last_kernel_ms(k, group_ms, pairing_ms); }

extern "C" int cg_verify_batch(cg_pvk* k, const uint8_t* inputs, uint64_t n_inputs, const uint8_t* proofs, uint64_t n,
                               uint8_t* verdicts) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    if (n_inputs != k->n_inputs)                           // SynthesisError::MalformedVerifyingKey (verifier.rs:30-32)
        return fail(CG_ERR_MALFORMED_KEY, "%llu public inputs for a key with gamma_abc_g1.len() = %llu",
                    (unsigned long long)n_inputs, (unsigned long long)(k->n_inputs + 1));
    if (n == 0) return CG_OK;
    if (!proofs || !verdicts || (n_inputs && !inputs)) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    try {
        std::lock_guard<std::mutex> lk(k->mu);
        CG_HIP(hipSetDevice(k->device));
        const uint64_t ell = n_inputs;
        const uint64_t chunk = n < VCHUNK ? n : VCHUNK;
        k->b_inputs.reserve(chunk, ell * 32);
        for (RowBuf* b : {&k->b_proofs, &k->b_status, &k->b_verdict, &k->b_in_g2}) b->reserve(chunk);
        grow(k->b_part, chunk * ell + 1);
        grow(k->b_parsed, chunk);
        grow(k->b_miller, chunk);
        k->timer.reset();
        for (uint64_t off = 0; off < n; off += chunk) {
            const uint64_t m = n - off < chunk ? n - off : chunk;
            k->b_inputs.up(k->st, inputs, off, m);
            k->proofs_up(proofs, off, m);
            k->timer.mark(0, k->st);
            if (ell) {
                k_vfy_inputs<<<ceil_div(m * ell, VBLOCK), VBLOCK, 0, k->st>>>(k->b_inputs.words(), m, (uint32_t)ell, k->tab.p, k->b_part.p);
                CG_KERNEL_CHECK();
            }
            k->check(m, k->b_inputs.words(), (uint32_t)ell);
            k->timer.mark(1, k->st);
            k->pairing(m);
            k->timer.mark(2, k->st);
            k->b_verdict.down(k->st, verdicts, off, m);
            CG_HIP(hipStreamSynchronize(k->st));
            k->timer.add();
        }
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}

// ---- one call's io_types layout, shared by the verifier and the creator of showings -------------------------------------
namespace {
struct IoLayout {
    std::vector<uint32_t> rev, com, hid;     // the inputs of each PublicIOType, ascending
    // the table each DLogPoK response walks, in the order dlog.rs:60-67 and :135-145 meet the bases: (gamma_abc[i+1], delta_g1)
    // per committed input, then the hidden inputs, then delta_g1 (table n_io is delta_g1's)
    std::vector<uint32_t> resp_tab;
};
// 0, or the failure already recorded.  This is the part that needs no key (cg_show_rand_count, cg_show_respond_batch).
int io_layout(const uint8_t* io_types, uint64_t n_io, IoLayout& L) {
    if (n_io && !io_types) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    if (n_io >= MK_RAND / 4) return fail(CG_ERR_INVALID_ARGUMENT, "too many io types");
    for (uint64_t i = 0; i < n_io; ++i) {
        switch (io_types[i]) {
            case CG_IO_REVEALED: L.rev.push_back((uint32_t)i); break;
            case CG_IO_HIDDEN: L.hid.push_back((uint32_t)i); break;
            case CG_IO_COMMITTED: L.com.push_back((uint32_t)i); break;
            default: return fail(CG_ERR_INVALID_ARGUMENT, "io_types[%llu] = %u is no PublicIOType", (unsigned long long)i, io_types[i]);
        }
    }
    for (uint32_t i : L.com) {
        L.resp_tab.push_back(i);
        L.resp_tab.push_back((uint32_t)n_io);
    }
    L.resp_tab.insert(L.resp_tab.end(), L.hid.begin(), L.hid.end());
    L.resp_tab.push_back((uint32_t)n_io);
    return CG_OK;
}
// under a key: the length first, then the types
int io_layout(const cg_pvk* k, const uint8_t* io_types, uint64_t n_io, IoLayout& L) {
    if (n_io != k->n_inputs)
        return fail(CG_ERR_MALFORMED_KEY, "%llu io types for a key with gamma_abc_g1.len() = %llu", (unsigned long long)n_io,
                    (unsigned long long)(k->n_inputs + 1));
    return io_layout(io_types, n_io, L);
}

}  // namespace

// ---- the internal entry (device_link.hpp): what cg_device_link_verify_batch needs of a key it cannot see into ----------------
namespace cg {
int pvk_link_view(cg_pvk* k, const uint8_t* io_types, uint64_t n_io, uint32_t pos0, uint32_t pos1, PvkLinkView& v) {
    IoLayout L;
    if (int rc = io_layout(k, io_types, n_io, L)) return rc;
    if (pos0 >= n_io || pos1 >= n_io) return fail(CG_ERR_INVALID_ARGUMENT, "pos0 = %u or pos1 = %u is no input of a key with %llu", pos0, pos1, (unsigned long long)n_io);
    if (io_types[pos0] != CG_IO_COMMITTED || io_types[pos1] != CG_IO_COMMITTED)
        return fail(CG_ERR_INVALID_ARGUMENT, "the device key's inputs %u and %u must both be committed inputs of the showing", pos0, pos1);
    if (pos0 == pos1) return fail(CG_ERR_INVALID_ARGUMENT, "pos0 and pos1 name the same input %u", pos0);
    auto ci = [&](uint32_t pos) { return (uint32_t)(std::find(L.com.begin(), L.com.end(), pos) - L.com.begin()); };
    pvk_link_handle(k, v);
    v.n_com = (uint32_t)L.com.size();
    v.ci0 = ci(pos0);
    v.ci1 = ci(pos1);
    return CG_OK;
}
void pvk_link_handle(cg_pvk* k, PvkLinkView& v) {
    v = PvkLinkView{&k->mu, k->device, k->st, k->tab.p, k->base_bytes.data(), k->n_inputs, 0, 0, 0, &k->dl_state, &k->dl_free,
                    &k->dlm_state, &k->dlm_free, &k->hq_state, &k->hq_free, &k->p256_state, &k->p256_free};
}
}  // namespace cg

namespace {
// the verifier's shape and tab_of: the revealed inputs, then (with a DLogPoK) the responses
ShowShape show_shape(const IoLayout& L, bool pok, std::vector<uint32_t>& tab_of) {
    ShowShape sh;
    sh.n_rev = (uint32_t)L.rev.size();
    sh.n_com = (uint32_t)L.com.size();
    sh.n_resp = (uint32_t)L.resp_tab.size();
    sh.n_fixed = sh.n_rev + (pok ? sh.n_resp : 0);
    sh.n_var = pok ? sh.n_com + 1 : 0;
    sh.n_terms = sh.n_fixed + sh.n_var;
    tab_of = L.rev;
    if (pok) tab_of.insert(tab_of.end(), L.resp_tab.begin(), L.resp_tab.end());
    return sh;
}

MkShape mk_shape(const IoLayout& L, uint64_t n_io) {
    MkShape sh;
    sh.n_io = (uint32_t)n_io;
    sh.n_com = (uint32_t)L.com.size();
    sh.n_resp = (uint32_t)L.resp_tab.size();
    sh.n_rand = 3 + sh.n_com + sh.n_resp;
    sh.n_fix = 2 * sh.n_resp + 1;
    sh.n_terms = sh.n_fix + 2;
    sh.n_out = 2 * sh.n_com + 5;
    return sh;
}
// the creator's desc: [table of term t | scalar of term t], as k_mk_fixed reads it
std::vector<uint32_t> mk_desc(const IoLayout& L, const MkShape& sh) {
    std::vector<uint32_t> desc = L.resp_tab, src;
    desc.insert(desc.end(), L.resp_tab.begin(), L.resp_tab.end());               // the nonces walk the same tables
    desc.push_back(sh.n_io + 1);                                                 // (acc_r + z)·G
    for (uint32_t c = 0; c < sh.n_com; ++c) {                     // (x_i, r_i) on (gamma_abc[i+1], delta_g1)
        src.push_back(L.com[c]);
        src.push_back(MK_RAND | (2 + c));
    }
    src.insert(src.end(), L.hid.begin(), L.hid.end());
    src.push_back(MK_RAND | (2 + sh.n_com));                                     // z on delta_g1
    for (uint32_t t = 0; t < sh.n_resp; ++t) src.push_back(MK_RAND | (3 + sh.n_com + t));
    src.push_back(0);                                                            // the last lane forms its own scalar
    desc.insert(desc.end(), src.begin(), src.end());
    return desc;
}
}  // namespace

extern "C" int cg_verify_show_batch(cg_pvk* k, const uint8_t* io_types, uint64_t n_io, const uint8_t* revealed,
                                    const uint8_t* rand_proofs, const uint8_t* com_hidden, const uint8_t* committed,
                                    const uint8_t* pok_c, const uint8_t* pok_s, uint64_t n, uint8_t* verdicts, uint8_t* k_out) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    IoLayout L;
    if (int rc = io_layout(k, io_types, n_io, L)) return rc;
    if (n == 0) return CG_OK;
    const bool pok = pok_c != nullptr;
    std::vector<uint32_t> tab_of;            // which table each fixed-base term walks
    const ShowShape sh = show_shape(L, pok, tab_of);
    if (!rand_proofs || !com_hidden || !verdicts || (sh.n_rev && !revealed) || (sh.n_com && !committed) || (pok && (!pok_s || !k_out)))
        return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    try {
        std::lock_guard<std::mutex> lk(k->mu);
        CG_HIP(hipSetDevice(k->device));
        const uint64_t chunk = n < VCHUNK ? n : VCHUNK;
        const uint32_t n_stmt = sh.n_com + 1;
        for (RowBuf* b : {&k->b_proofs, &k->b_status, &k->b_verdict, &k->b_in_g2, &k->b_comh, &k->b_chal}) b->reserve(chunk);
        k->b_inputs.reserve(chunk, sh.n_rev * 32);
        k->b_comm.reserve(chunk, sh.n_com * 64);
        k->b_rows.reserve(chunk, sh.n_resp * 32);
        k->b_k.reserve(chunk, n_stmt * 32);
        grow(k->b_parsed, chunk);
        grow(k->b_miller, chunk);
        grow(k->b_part, chunk * sh.n_terms + 1);
        grow(k->b_desc, tab_of.size() + 1);
        h2d_sync(k->b_desc.p, tab_of.data(), tab_of.size() * sizeof(uint32_t), k->st);
        k->timer.reset();
        for (uint64_t off = 0; off < n; off += chunk) {
            const uint64_t m = n - off < chunk ? n - off : chunk;
            k->proofs_up(rand_proofs, off, m);
            k->b_comh.up(k->st, com_hidden, off, m);
            k->b_inputs.up(k->st, revealed, off, m);
            k->b_comm.up(k->st, committed, off, m);
            if (pok) {
                k->b_chal.up(k->st, pok_c, off, m);
                k->b_rows.up(k->st, pok_s, off, m);
            }
            const uint32_t *d_rev = k->b_inputs.words(), *d_s = k->b_rows.words(), *d_c = k->b_chal.words(), *d_comh = k->b_comh.words(),
                           *d_comm = k->b_comm.words();
            k->timer.mark(0, k->st);
            if (sh.n_terms) {
                const uint32_t blocks = ceil_div(m * sh.n_fixed, VBLOCK) + ceil_div(m * sh.n_var, VBLOCK);
                k_show_terms<<<blocks, VBLOCK, 0, k->st>>>(d_rev, d_s, d_c, d_comh, d_comm, m, sh, k->b_desc.p, k->tab.p, k->b_part.p);
                CG_KERNEL_CHECK();
            }
            const uint32_t grid = ceil_div(m, VBLOCK);
            k->check(m, d_rev, 0u);
            k_show_check<<<grid, VBLOCK, 0, k->st>>>(d_rev, d_s, d_c, d_comh, d_comm, m, sh, k->b_part.p, k->g0, k->b_parsed.p,
                                                     k->b_status.bytes());
            CG_KERNEL_CHECK();
            // k_show_k writes zeros for a malformed showing: in the latency arrangement the status is final only after the
            // pairing has met the subgroup chain, so the k points follow it there
            auto show_k = [&] {
                if (!pok) return;
                k_show_k<<<ceil_div(m * n_stmt, VBLOCK), VBLOCK, 0, k->st>>>(m, sh, k->b_part.p, k->b_status.bytes(), k->b_k.words_mut());
                CG_KERNEL_CHECK();
            };
            if (!k->latency) show_k();
            k->timer.mark(1, k->st);
            k->pairing(m);
            if (k->latency) show_k();
            k->timer.mark(2, k->st);
            k->b_verdict.down(k->st, verdicts, off, m);
            if (pok) k->b_k.down(k->st, k_out, off, m);
            CG_HIP(hipStreamSynchronize(k->st));
            k->timer.add();
        }
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}

extern "C" int cg_pvk_set_showings_overlap(cg_pvk* k, int32_t on) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    if (on != 0 && on != 1) return fail(CG_ERR_INVALID_ARGUMENT, "overlap is 0 or 1, not %d", on);
    std::lock_guard<std::mutex> lk(k->mu);
    k->overlap = on != 0;
    return CG_OK;
}

// ---- what the two whole-showing entries check and build alike, on the host --------------------------------------------------
namespace {
// the DLogPoK's context as cg_dlog_challenge_batch takes it: CG_OK, or the failure already recorded
int check_context(const uint8_t* context, uint64_t context_len, uint64_t context_stride) {
    if (context_len && !context) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    if (context_stride && context_stride < context_len)
        return fail(CG_ERR_INVALID_ARGUMENT, "a context stride of %llu is shorter than the context's %llu bytes", (unsigned long long)context_stride,
                    (unsigned long long)context_len);
    if (context_len > 0xffffffffull - 8) return fail(CG_ERR_INVALID_ARGUMENT, "a context of %llu bytes is longer than a Merlin message", (unsigned long long)context_len);
    return CG_OK;
}
// every link's slot holds gamma_abc_g1[pos] ‖ delta_g1 of this key; slot_bytes(slot) is the range key's registered 128 bytes or
// null, `add_bases` the call that registers them.  Under both locks
template <class SlotBytes>
int check_link_slots(const cg_pvk* k, const IoLayout& L, uint64_t n_io, uint32_t n_ranges, const cg_show_range_link* links, SlotBytes slot_bytes,
                     const char* add_bases) {
    const uint8_t* delta = k->base_bytes.data() + 64 * n_io;
    for (uint32_t j = 0; j < n_ranges; ++j) {
        const uint8_t* reg = slot_bytes(links[j].slot);
        if (!reg) return fail(CG_ERR_INVALID_ARGUMENT, "link %u: slot %u was not registered on the range key (%s)", j, links[j].slot, add_bases);
        const uint32_t input = L.com[links[j].committed_index];
        if (memcmp(reg, k->base_bytes.data() + 64 * (uint64_t)input, 64) || memcmp(reg + 64, delta, 64))
            return fail(CG_ERR_INVALID_ARGUMENT, "link %u: slot %u does not hold gamma_abc_g1[%u] and delta_g1 of this key", j, links[j].slot, input + 1);
    }
    return CG_OK;
}
// the bases as the DLogPoK's transcript absorbs them, in the order the responses meet them
std::vector<uint32_t> compressed_bases(const cg_pvk* k, const IoLayout& L) {
    std::vector<uint32_t> bases_cmp(8 * L.resp_tab.size());
    for (size_t t = 0; t < L.resp_tab.size(); ++t) {
        uint32_t w[16];
        memcpy(w, k->base_bytes.data() + 64 * (uint64_t)L.resp_tab[t], 64);
        ml_compress_g1(w, bases_cmp.data() + 8 * t);
    }
    return bases_cmp;
}
// a chunk's contexts, one per showing: the caller's last context ends with its bytes, not with its stride
void contexts_up(cg_pvk* k, const uint8_t* context, uint64_t context_len, uint64_t context_stride, uint64_t off, uint64_t m) {
    if (context_stride && context_len)
        CG_HIP(hipMemcpyAsync(k->b_ctx.bytes(), context + off * context_stride, (m - 1) * context_stride + context_len, hipMemcpyHostToDevice, k->st));
}
}  // namespace

// `verify_show`'s cryptographic checks (creds/src/lib.rs:630-658, :832-890) for a batch of showings of one layout: the
// kernels of cg_verify_show_batch, k_show_challenge behind k_show_k, k_show_link into memory the range key's kernels read
// (rangeverify.hpp's internal entry, on the range key's stream behind an event), k_show_verdict.  Per chunk nothing comes
// down between the steps.  The locks are taken in the order cg_pvk, cg_range_vk.
extern "C" int cg_verify_showings_batch(cg_pvk* k, cg_range_vk* rk, const uint8_t* io_types, uint64_t n_io, const uint8_t* context,
                                        uint64_t context_len, uint64_t context_stride, const uint8_t* revealed, const uint8_t* rand_proofs,
                                        const uint8_t* com_hidden, const uint8_t* committed, const uint8_t* pok_c, const uint8_t* pok_s,
                                        uint32_t n_ranges, const cg_show_range_link* links, const uint8_t* shifts, const cg_range_rows* ranges,
                                        uint64_t n, uint8_t* verdicts, uint8_t* part_verdicts) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    IoLayout L;
    if (int rc = io_layout(k, io_types, n_io, L)) return rc;
    if (n == 0) return CG_OK;
    std::vector<uint32_t> desc;              // tab_of of k_show_terms, then k_show_link's: the committed index and the table per range
    const ShowShape sh = show_shape(L, true, desc);
    const uint32_t n_tab_of = (uint32_t)desc.size(), n_stmt = sh.n_com + 1;
    if (!rand_proofs || !com_hidden || !verdicts || !pok_c || !pok_s || (sh.n_rev && !revealed) || (sh.n_com && !committed) ||
        (n_ranges && (!rk || !links || !shifts || !ranges)))
        return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = check_context(context, context_len, context_stride)) return rc;
    for (uint32_t j = 0; j < n_ranges; ++j) {
        const cg_range_rows& r = ranges[j];
        if (!r.com_f || !r.com_g || !r.com_q || !r.evals || !r.proofs || !r.randomizers || !r.pok_c || !r.pok_s)
            return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
        if (links[j].committed_index >= sh.n_com)
            return fail(CG_ERR_INVALID_ARGUMENT, "link %u: committed_index %u of %u committed inputs", j, links[j].committed_index, sh.n_com);
    }
    for (uint32_t j = 0; j < n_ranges; ++j) desc.push_back(links[j].committed_index);
    for (uint32_t j = 0; j < n_ranges; ++j) desc.push_back(L.com[links[j].committed_index]);
    try {
        std::lock_guard<std::mutex> lk(k->mu);
        std::unique_lock<std::mutex> lr;
        if (n_ranges) {
            lr = std::unique_lock<std::mutex>(range_vk_lock(rk));
            if (range_vk_device(rk) != k->device)
                return fail(CG_ERR_INVALID_ARGUMENT, "the Groth16 key is on device %d and the range key on device %d", k->device, range_vk_device(rk));
        }
        if (int rc = check_link_slots(k, L, n_io, n_ranges, links, [&](uint32_t slot) { return range_vk_slot_bytes(rk, slot); }, "cg_range_vk_add_bases"))
            return rc;
        const std::vector<uint32_t> bases_cmp = compressed_bases(k, L);
        CG_HIP(hipSetDevice(k->device));
        const uint64_t chunk = n < VCHUNK ? n : VCHUNK;
        for (RowBuf* b : {&k->b_proofs, &k->b_status, &k->b_verdict, &k->b_in_g2, &k->b_comh, &k->b_chal, &k->b_cprime, &k->b_same, &k->b_final})
            b->reserve(chunk);
        k->b_inputs.reserve(chunk, sh.n_rev * 32);
        k->b_comm.reserve(chunk, sh.n_com * 64);
        k->b_rows.reserve(chunk, sh.n_resp * 32);
        k->b_k.reserve(chunk, n_stmt * 32);
        k->b_ycmp.reserve(chunk, n_stmt * 32);
        k->b_shift.reserve(chunk, n_ranges * 32);
        k->b_link.reserve(chunk, n_ranges * 64);
        k->b_rverd.reserve(chunk, n_ranges);
        k->b_parts.reserve(chunk, n_ranges + 1);
        if (context_stride) k->b_ctx.reserve(chunk, context_stride);
        else k->b_ctx.reserve(1, context_len);
        grow(k->b_parsed, chunk);
        grow(k->b_miller, chunk);
        grow(k->b_part, chunk * sh.n_terms + 1);
        grow(k->b_desc, desc.size() + 1);
        grow(k->b_bases_cmp, bases_cmp.size() * sizeof(uint32_t));
        h2d_sync(k->b_desc.p, desc.data(), desc.size() * sizeof(uint32_t), k->st);
        h2d_sync(k->b_bases_cmp.p, bases_cmp.data(), bases_cmp.size() * sizeof(uint32_t), k->st);
        if (!context_stride) k->b_ctx.up(k->st, context, 0, 1);
        if (n_ranges) range_vk_reserve(rk, chunk);
        k->timer.reset();
        for (uint64_t off = 0; off < n; off += chunk) {
            const uint64_t m = n - off < chunk ? n - off : chunk;
            k->proofs_up(rand_proofs, off, m);
            k->b_comh.up(k->st, com_hidden, off, m);
            k->b_inputs.up(k->st, revealed, off, m);
            k->b_comm.up(k->st, committed, off, m);
            k->b_chal.up(k->st, pok_c, off, m);
            k->b_rows.up(k->st, pok_s, off, m);
            k->b_shift.up(k->st, shifts, off, m);
            contexts_up(k, context, context_len, context_stride, off, m);
            const uint32_t *d_rev = k->b_inputs.words(), *d_s = k->b_rows.words(), *d_c = k->b_chal.words(), *d_comh = k->b_comh.words(),
                           *d_comm = k->b_comm.words();
            const uint32_t grid = ceil_div(m, VBLOCK);
            // the range half: every range on the range key's stream, behind the event recorded on ours
            auto range_half = [&] {
                if (!n_ranges) return;
                CG_HIP(hipEventRecord(k->ev_link, k->st));
                CG_HIP(hipStreamWaitEvent(range_vk_stream(rk), k->ev_link, 0));
                for (uint32_t j = 0; j < n_ranges; ++j)
                    range_vk_enqueue(rk, links[j].slot, ranges[j], off, m, k->b_link.words() + 16 * (uint64_t)j * m, k->b_rverd.bytes() + (uint64_t)j * m);
                CG_HIP(hipEventRecord(k->ev_ranges, range_vk_stream(rk)));
            };
            if (n_ranges) {
                k_show_link<<<ceil_div(m * n_ranges, VBLOCK), VBLOCK, 0, k->st>>>(d_comm, k->b_shift.words(), m, sh.n_com, n_ranges, k->b_desc.p + n_tab_of,
                                                                                 k->tab.p, k->b_link.words_mut());
                CG_KERNEL_CHECK();
            }
            if (k->overlap) range_half();
            // the Groth16 half, as cg_verify_show_batch runs it
            const uint32_t blocks = ceil_div(m * sh.n_fixed, VBLOCK) + ceil_div(m * sh.n_var, VBLOCK);
            k_show_terms<<<blocks, VBLOCK, 0, k->st>>>(d_rev, d_s, d_c, d_comh, d_comm, m, sh, k->b_desc.p, k->tab.p, k->b_part.p);
            CG_KERNEL_CHECK();
            k->check(m, d_rev, 0u);
            k_show_check<<<grid, VBLOCK, 0, k->st>>>(d_rev, d_s, d_c, d_comh, d_comm, m, sh, k->b_part.p, k->g0, k->b_parsed.p, k->b_status.bytes());
            CG_KERNEL_CHECK();
            auto show_k = [&] {
                k_show_k<<<ceil_div(m * n_stmt, VBLOCK), VBLOCK, 0, k->st>>>(m, sh, k->b_part.p, k->b_status.bytes(), k->b_k.words_mut());
                CG_KERNEL_CHECK();
            };
            if (!k->latency) show_k();
            k->pairing(m);
            if (k->latency) show_k();             // the status is final only behind the pairing there (cg_verify_show_batch)
            k_show_challenge<<<grid, VBLOCK, 0, k->st>>>(d_comh, d_comm, d_c, m, sh, k->b_bases_cmp.p, k->b_k.words(), k->b_ctx.bytes(), context_len,
                                                        context_stride, k->b_status.bytes(), k->b_ycmp.words_mut(), k->b_cprime.words_mut(),
                                                        k->b_same.bytes(), k->b_verdict.bytes());
            CG_KERNEL_CHECK();
            if (!k->overlap) range_half();
            if (n_ranges) CG_HIP(hipStreamWaitEvent(k->st, k->ev_ranges, 0));
            k_show_verdict<<<grid, VBLOCK, 0, k->st>>>(k->b_verdict.bytes(), k->b_rverd.bytes(), m, n_ranges, k->b_parts.bytes(), k->b_final.bytes());
            CG_KERNEL_CHECK();
            k->b_final.down(k->st, verdicts, off, m);
            k->b_parts.down(k->st, part_verdicts, off, m);
            CG_HIP(hipStreamSynchronize(k->st));
        }
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}

// `create_show_proof`'s curve arithmetic and transcripts (creds/src/lib.rs:364-373, :468-471, :505-509) for a batch of client
// states of one layout.  Per chunk of VCHUNK states the kernels run in the order of this file's head; the range half walks
// the chunk in pieces of RANGE_PK_PIECE on the range key's stream (rangeproof.hpp), reading the openings and ped_com where
// k_mk_shift wrote them and bringing its proof rows down itself.  With the overlap on it waits for an event recorded right
// behind k_mk_shift and so runs beside k_mk_var, which it does not need; with it off, for one recorded behind k_mk_respond.
// Either way the range half is put on its stream after every Groth16 kernel is on ours: its copies to the caller's memory
// may hold the host.  Our stream waits for the range stream's last copy before k_mk_parts.  The locks are taken in the
// order cg_pvk, cg_range_pk.
extern "C" int cg_create_showings_batch(cg_pvk* k, cg_range_pk* rk, const uint8_t* io_types, uint64_t n_io, const uint8_t* context,
                                        uint64_t context_len, uint64_t context_stride, const uint8_t* proofs, const uint8_t* inputs,
                                        const uint8_t* rand, uint32_t n_ranges, const cg_show_range_link* links, const uint8_t* shifts,
                                        const uint8_t* range_rand, uint64_t n, uint8_t* rand_proofs, uint8_t* com_hidden, uint8_t* committed,
                                        uint8_t* pok_c, uint8_t* pok_s, const cg_range_made* ranges, uint8_t* status, uint8_t* part_status) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    IoLayout L;
    if (int rc = io_layout(k, io_types, n_io, L)) return rc;
    if (!k->gamma_is_one)
        return fail(CG_ERR_MALFORMED_KEY, "gamma_g2 is not the G2 generator: C - (acc_r + z) G re-randomises gamma = 1 keys only");
    if (n == 0) return CG_OK;
    const MkShape sh = mk_shape(L, n_io);
    if (!proofs || !rand || !rand_proofs || !com_hidden || !pok_c || !pok_s || !status || (sh.n_resp > 1 && !inputs) || (sh.n_com && !committed) ||
        (n_ranges && (!rk || !links || !shifts || !range_rand || !ranges)))
        return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = check_context(context, context_len, context_stride)) return rc;
    for (uint32_t j = 0; j < n_ranges; ++j) {
        const cg_range_made& r = ranges[j];
        if (!r.com_f || !r.com_g || !r.com_q || !r.evals || !r.proofs || !r.pok_c || !r.pok_s) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
        if (links[j].committed_index >= sh.n_com)
            return fail(CG_ERR_INVALID_ARGUMENT, "link %u: committed_index %u of %u committed inputs", j, links[j].committed_index, sh.n_com);
    }
    std::vector<uint32_t> desc = mk_desc(L, sh);                  // then k_mk_shift's: the committed index and the input per range
    const uint32_t n_mk_desc = (uint32_t)desc.size(), n_stmt = sh.n_com + 1;
    for (uint32_t j = 0; j < n_ranges; ++j) desc.push_back(links[j].committed_index);
    for (uint32_t j = 0; j < n_ranges; ++j) desc.push_back(L.com[links[j].committed_index]);
    try {
        std::lock_guard<std::mutex> lk(k->mu);
        std::unique_lock<std::mutex> lr;
        if (n_ranges) {
            lr = std::unique_lock<std::mutex>(range_pk_lock(rk));
            if (range_pk_device(rk) != k->device)
                return fail(CG_ERR_INVALID_ARGUMENT, "the Groth16 key is on device %d and the range key on device %d", k->device, range_pk_device(rk));
        }
        if (int rc = check_link_slots(k, L, n_io, n_ranges, links, [&](uint32_t slot) { return range_pk_slot_bytes(rk, slot); }, "cg_range_pk_add_bases"))
            return rc;
        const std::vector<uint32_t> bases_cmp = compressed_bases(k, L);
        CG_HIP(hipSetDevice(k->device));
        const uint64_t chunk = n < VCHUNK ? n : VCHUNK;
        for (RowBuf* b : {&k->b_proofs, &k->b_status, &k->b_rproofs, &k->b_comh, &k->b_cprime, &k->b_final}) b->reserve(chunk);
        k->b_inputs.reserve(chunk, sh.n_io * 32);
        k->b_rows.reserve(chunk, sh.n_rand * 32);
        k->b_comm.reserve(chunk, sh.n_com * 64);
        k->b_k.reserve(chunk, n_stmt * 32);
        k->b_ycmp.reserve(chunk, n_stmt * 32);
        k->b_resp.reserve(chunk, sh.n_resp * 32);
        k->b_shift.reserve(chunk, n_ranges * 32);
        k->b_lopen.reserve(chunk, n_ranges * 64);
        k->b_link.reserve(chunk, n_ranges * 64);
        k->b_lmade.reserve(chunk, n_ranges);
        k->b_rverd.reserve(chunk, n_ranges);
        k->b_parts.reserve(chunk, n_ranges + 1);
        if (context_stride) k->b_ctx.reserve(chunk, context_stride);
        else k->b_ctx.reserve(1, context_len);
        grow(k->b_part, chunk * sh.n_terms + 1);
        grow(k->b_part_g2, chunk);
        grow(k->b_desc, desc.size());
        grow(k->b_bases_cmp, bases_cmp.size() * sizeof(uint32_t));
        h2d_sync(k->b_desc.p, desc.data(), desc.size() * sizeof(uint32_t), k->st);
        h2d_sync(k->b_bases_cmp.p, bases_cmp.data(), bases_cmp.size() * sizeof(uint32_t), k->st);
        if (!context_stride) k->b_ctx.up(k->st, context, 0, 1);
        if (n_ranges) range_pk_reserve(rk, chunk);
        k->timer.reset();                     // the two handles' stages interleave: nothing is timed
        const uint64_t rand_pitch = (uint64_t)n_ranges * CG_RANGE_N_RAND * 32;
        for (uint64_t off = 0; off < n; off += chunk) {
            const uint64_t m = n - off < chunk ? n - off : chunk;
            k->b_proofs.up(k->st, proofs, off, m);
            k->b_inputs.up(k->st, inputs, off, m);
            k->b_rows.up(k->st, rand, off, m);
            k->b_shift.up(k->st, shifts, off, m);
            contexts_up(k, context, context_len, context_stride, off, m);
            const uint32_t *d_pr = k->b_proofs.words(), *d_in = k->b_inputs.words(), *d_rd = k->b_rows.words();
            uint8_t* d_status = k->b_status.bytes();
            const uint32_t grid = ceil_div(m, VBLOCK);
            auto out = [&](uint32_t o_lo, uint32_t o_n) {
                k_mk_out<<<ceil_div(m * o_n, VBLOCK), VBLOCK, 0, k->st>>>(d_pr, m, sh, o_lo, o_n, k->b_part.p, k->b_part_g2.p, d_status,
                                                                         k->b_rproofs.words_mut(), k->b_comh.words_mut(), k->b_comm.words_mut(),
                                                                         k->b_k.words_mut());
                CG_KERNEL_CHECK();
            };
            k_mk_check<<<grid, VBLOCK, 0, k->st>>>(d_pr, d_in, d_rd, m, sh, k->b_desc.p, d_status);
            CG_KERNEL_CHECK();
            k_mk_fixed<<<ceil_div(m * sh.n_fix, VBLOCK), VBLOCK, 0, k->st>>>(d_in, d_rd, m, sh, k->b_desc.p, k->tab.p, k->b_part.p);
            CG_KERNEL_CHECK();
            out(3u, sh.n_out - 3);                                // com_hidden, committed, k: the fixed-base partials alone
            if (n_ranges) {
                k_mk_shift<<<ceil_div(m * n_ranges, VBLOCK), VBLOCK, 0, k->st>>>(d_in, d_rd, k->b_comm.words(), k->b_shift.words(), d_status, m, sh, n_ranges,
                                                                                k->b_desc.p + n_mk_desc, k->tab.p, k->b_lopen.words_mut(),
                                                                                k->b_link.words_mut(), k->b_lmade.bytes());
                CG_KERNEL_CHECK();
                if (k->overlap) CG_HIP(hipEventRecord(k->ev_link, k->st));
            }
            k_mk_var<<<ceil_div(2 * m, VBLOCK) + grid, VBLOCK, 0, k->st>>>(d_pr, d_rd, m, sh, k->tab_g2.p, k->b_part.p, k->b_part_g2.p);
            CG_KERNEL_CHECK();
            out(0u, 3u);                                          // A', B', C''
            k_mk_challenge<<<grid, VBLOCK, 0, k->st>>>(k->b_comh.words(), k->b_comm.words(), m, sh, k->b_bases_cmp.p, k->b_k.words(), k->b_ctx.bytes(),
                                                      context_len, context_stride, d_status, k->b_ycmp.words_mut(), k->b_cprime.words_mut());
            CG_KERNEL_CHECK();
            k_mk_respond<<<ceil_div(m * sh.n_resp, VBLOCK), VBLOCK, 0, k->st>>>(d_in, d_rd, k->b_cprime.words(), m, sh, k->b_desc.p, d_status,
                                                                               k->b_resp.words_mut());
            CG_KERNEL_CHECK();
            if (n_ranges) {
                if (!k->overlap) CG_HIP(hipEventRecord(k->ev_link, k->st));
                hipStream_t rst = range_pk_stream(rk);
                CG_HIP(hipStreamWaitEvent(rst, k->ev_link, 0));
                for (uint32_t j = 0; j < n_ranges; ++j) {
                    const cg_range_made& r = ranges[j];
                    const RangePkOut ro{r.com_f, r.com_g, r.com_q, r.evals, r.proofs, r.pok_c, r.pok_s, r.challenges, nullptr};
                    for (uint64_t po = 0; po < m; po += RANGE_PK_PIECE) {
                        const uint64_t mm = m - po < RANGE_PK_PIECE ? m - po : RANGE_PK_PIECE;
                        const uint64_t row = (uint64_t)j * m + po;
                        range_pk_enqueue(rk, links[j].slot, k->b_lopen.words() + 16 * row, k->b_link.words() + 16 * row,
                                         range_rand + (off + po) * rand_pitch + (uint64_t)j * CG_RANGE_N_RAND * 32, rand_pitch, ro, off + po, mm,
                                         k->b_rverd.bytes() + row);
                    }
                }
                CG_HIP(hipEventRecord(k->ev_ranges, rst));
                CG_HIP(hipStreamWaitEvent(k->st, k->ev_ranges, 0));
            }
            k_mk_parts<<<grid, VBLOCK, 0, k->st>>>(d_status, k->b_lmade.bytes(), k->b_rverd.bytes(), m, n_ranges, k->b_parts.bytes(), k->b_final.bytes());
            CG_KERNEL_CHECK();
            k->b_rproofs.down(k->st, rand_proofs, off, m);
            k->b_comh.down(k->st, com_hidden, off, m);
            k->b_comm.down(k->st, committed, off, m);
            k->b_cprime.down(k->st, pok_c, off, m);
            k->b_resp.down(k->st, pok_s, off, m);
            k->b_final.down(k->st, status, off, m);
            k->b_parts.down(k->st, part_status, off, m);
            CG_HIP(hipStreamSynchronize(k->st));
        }
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}

// The creating side's link (creds/src/lib.rs:370-372, :468-470, :505-507): k_show_shift over the table of one input
extern "C" int cg_show_shift_batch(cg_pvk* k, uint32_t input_index, const uint8_t* openings, const uint8_t* commitments, const uint8_t* shifts,
                                   uint64_t n, uint8_t* openings_out, uint8_t* ped_com_out, uint8_t* status) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    if (input_index >= k->n_inputs)
        return fail(CG_ERR_INVALID_ARGUMENT, "input %u of a key with %llu public inputs", input_index, (unsigned long long)k->n_inputs);
    if (n == 0) return CG_OK;
    if (!openings || !commitments || !shifts || !openings_out || !ped_com_out || !status) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    try {
        std::lock_guard<std::mutex> lk(k->mu);
        CG_HIP(hipSetDevice(k->device));
        const uint64_t chunk = n < VCHUNK ? n : VCHUNK;
        for (RowBuf* b : {&k->b_comh, &k->b_chal, &k->b_status}) b->reserve(chunk);
        k->b_rows.reserve(chunk, 64);
        k->b_inputs.reserve(chunk, 64);
        k->b_link.reserve(chunk, 64);
        for (uint64_t off = 0; off < n; off += chunk) {
            const uint64_t m = n - off < chunk ? n - off : chunk;
            k->b_rows.up(k->st, openings, off, m);
            k->b_comh.up(k->st, commitments, off, m);
            k->b_chal.up(k->st, shifts, off, m);
            k_show_shift<<<ceil_div(m, VBLOCK), VBLOCK, 0, k->st>>>(k->b_rows.words(), k->b_comh.words(), k->b_chal.words(), m,
                                                                   k->tab.p + (uint64_t)input_index * FB_NWIN * FB_WIN, k->b_inputs.words_mut(),
                                                                   k->b_link.words_mut(), k->b_status.bytes());
            CG_KERNEL_CHECK();
            k->b_inputs.down(k->st, openings_out, off, m);
            k->b_link.down(k->st, ped_com_out, off, m);
            k->b_status.down(k->st, status, off, m);
            CG_HIP(hipStreamSynchronize(k->st));
        }
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}

extern "C" int cg_show_rand_count(const uint8_t* io_types, uint64_t n_io, uint64_t* n_rand) {
    if (!n_rand) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    IoLayout L;
    if (int rc = io_layout(io_types, n_io, L)) return rc;
    *n_rand = mk_shape(L, n_io).n_rand;
    return CG_OK;
}

extern "C" int cg_show_commit_batch(cg_pvk* k, const uint8_t* io_types, uint64_t n_io, const uint8_t* proofs, const uint8_t* inputs,
                                    const uint8_t* rand, uint64_t n, uint8_t* rand_proofs, uint8_t* com_hidden, uint8_t* committed,
                                    uint8_t* k_out, uint8_t* status) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    IoLayout L;
    if (int rc = io_layout(k, io_types, n_io, L)) return rc;
    if (!k->gamma_is_one)
        return fail(CG_ERR_MALFORMED_KEY, "gamma_g2 is not the G2 generator: C - (acc_r + z) G re-randomises gamma = 1 keys only");
    if (n == 0) return CG_OK;
    const MkShape sh = mk_shape(L, n_io);
    if (!proofs || !rand || !rand_proofs || !com_hidden || !k_out || !status || (sh.n_resp > 1 && !inputs) || (sh.n_com && !committed))
        return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    const std::vector<uint32_t> desc = mk_desc(L, sh);
    try {
        std::lock_guard<std::mutex> lk(k->mu);
        CG_HIP(hipSetDevice(k->device));
        const uint64_t chunk = n < VCHUNK ? n : VCHUNK;
        const uint32_t n_stmt = sh.n_com + 1;
        for (RowBuf* b : {&k->b_proofs, &k->b_status, &k->b_rproofs, &k->b_comh}) b->reserve(chunk);
        k->b_inputs.reserve(chunk, sh.n_io * 32);
        k->b_rows.reserve(chunk, sh.n_rand * 32);
        k->b_comm.reserve(chunk, sh.n_com * 64);
        k->b_k.reserve(chunk, n_stmt * 32);
        grow(k->b_part, chunk * sh.n_terms + 1);
        grow(k->b_part_g2, chunk);
        grow(k->b_desc, desc.size());
        h2d_sync(k->b_desc.p, desc.data(), desc.size() * sizeof(uint32_t), k->st);
        for (uint64_t off = 0; off < n; off += chunk) {
            const uint64_t m = n - off < chunk ? n - off : chunk;
            k->b_proofs.up(k->st, proofs, off, m);
            k->b_inputs.up(k->st, inputs, off, m);
            k->b_rows.up(k->st, rand, off, m);
            const uint32_t *d_pr = k->b_proofs.words(), *d_in = k->b_inputs.words(), *d_rd = k->b_rows.words();
            k_mk_check<<<ceil_div(m, VBLOCK), VBLOCK, 0, k->st>>>(d_pr, d_in, d_rd, m, sh, k->b_desc.p, k->b_status.bytes());
            CG_KERNEL_CHECK();
            k_mk_fixed<<<ceil_div(m * sh.n_fix, VBLOCK), VBLOCK, 0, k->st>>>(d_in, d_rd, m, sh, k->b_desc.p, k->tab.p, k->b_part.p);
            CG_KERNEL_CHECK();
            k_mk_var<<<ceil_div(2 * m, VBLOCK) + ceil_div(m, VBLOCK), VBLOCK, 0, k->st>>>(d_pr, d_rd, m, sh, k->tab_g2.p, k->b_part.p,
                                                                                         k->b_part_g2.p);
            CG_KERNEL_CHECK();
            k_mk_out<<<ceil_div(m * sh.n_out, VBLOCK), VBLOCK, 0, k->st>>>(d_pr, m, sh, 0u, sh.n_out, k->b_part.p, k->b_part_g2.p, k->b_status.bytes(),
                                                                          k->b_rproofs.words_mut(), k->b_comh.words_mut(),
                                                                          k->b_comm.words_mut(), k->b_k.words_mut());
            CG_KERNEL_CHECK();
            k->b_rproofs.down(k->st, rand_proofs, off, m);
            k->b_comh.down(k->st, com_hidden, off, m);
            k->b_comm.down(k->st, committed, off, m);
            k->b_k.down(k->st, k_out, off, m);
            k->b_status.down(k->st, status, off, m);
            CG_HIP(hipStreamSynchronize(k->st));
        }
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}

// DLogPoK::prove's responses (dlog.rs:101-109) once the host's transcript has produced c: plain host arithmetic
extern "C" int cg_show_respond_batch(const uint8_t* io_types, uint64_t n_io, const uint8_t* inputs, const uint8_t* rand,
                                     const uint8_t* pok_c, const uint8_t* status, uint64_t n, uint8_t* pok_s) {
    IoLayout L;
    if (int rc = io_layout(io_types, n_io, L)) return rc;
    if (n == 0) return CG_OK;
    const MkShape sh = mk_shape(L, n_io);
    if (!rand || !pok_c || !pok_s || (sh.n_resp > 1 && !inputs)) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    const std::vector<uint32_t> desc = mk_desc(L, sh);
    const uint32_t* src = desc.data() + sh.n_fix;
    auto secret = [&](uint64_t p, uint32_t t) {
        return src[t] & MK_RAND ? rand + 32 * (p * sh.n_rand + (src[t] & ~MK_RAND)) : inputs + 32 * (p * sh.n_io + src[t]);
    };
    auto nonce = [&](uint64_t p, uint32_t t) { return rand + 32 * (p * sh.n_rand + 3 + sh.n_com + t); };
    return dlog_respond(n, sh.n_resp, status, pok_c, secret, nonce, pok_s, "an input");
}

extern "C" void cg_pvk_free(cg_pvk* k) { free_handle(k); }

// prepare_verifying_key (verifier.rs:13-20) on the host: one pairing and two G2Prepared, written as ark-serialize writes a
// PreparedVerifyingKey (data_structures.rs:62-71): the VerifyingKey bytes as given, alpha_g1_beta_g2, gamma_g2_neg_pc,
// delta_g2_neg_pc.  pvk_out = NULL asks for the size only.
static void put_fq(std::vector<uint8_t>& o, const Fq& a) {
    uint8_t b[32];
    fp_to_bytes(from_mont(a), b);
    o.insert(o.end(), b, b + 32);
}
static void put_fq2(std::vector<uint8_t>& o, const Fq2& a) { put_fq(o, a.c0); put_fq(o, a.c1); }
static void put_g2_prepared(std::vector<uint8_t>& o, const G2Affine& q) {
    uint64_t n = q.is_inf() ? 0 : NC;
    const uint8_t* pn = (const uint8_t*)&n;
    o.insert(o.end(), pn, pn + 8);
    if (n) {
        std::vector<EllCoeff> c(NC);
        g2_prepare(q, c.data());
        for (const EllCoeff& e : c) { put_fq2(o, e.c0); put_fq2(o, e.c1); put_fq2(o, e.c2); }
    }
    o.push_back(q.is_inf() ? 1 : 0);
}

extern "C" int cg_prepare_verifying_key(const uint8_t* vk_bytes, uint64_t vk_len, uint8_t* pvk_out, uint64_t cap, uint64_t* len) {
    if (!vk_bytes || !len) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    try {
        HostVk vk;
        KeyRd r{vk_bytes, vk_len, 0};
        read_vk(r, vk);
        if (r.off != vk_len) throw HipError(CG_ERR_PARSE, "trailing bytes after VerifyingKey");
        const uint64_t need = vk_len + 384 + 2 * 9 + (vk.gamma_g2.is_inf() ? 0 : NC * 192) + (vk.delta_g2.is_inf() ? 0 : NC * 192);
        *len = need;
        if (!pvk_out) return CG_OK;
        if (cap < need) return fail(CG_ERR_INVALID_ARGUMENT, "output buffer too small (%llu bytes needed)", (unsigned long long)need);
        // alpha_g1_beta_g2 = E::pairing(alpha_g1, beta_g2)
        MillerPairs mp;
        mp.p[0] = vk.alpha_g1; mp.q[0] = vk.beta_g2; mp.tab[0] = nullptr;
        mp.live[0] = !vk.alpha_g1.is_inf() && !vk.beta_g2.is_inf();
        for (int j = 1; j < 3; ++j) { mp.p[j] = G1Affine::inf(); mp.q[j] = G2Affine::inf(); mp.tab[j] = nullptr; mp.live[j] = false; }
        Fq12 ab;
        if (!final_exponentiation(multi_miller_loop<1>(mp), ab)) throw HipError(CG_ERR_MALFORMED_KEY, "degenerate pairing");
        std::vector<uint8_t> o(vk_bytes, vk_bytes + vk_len);
        const Fq2* c[6] = {&ab.c0.c0, &ab.c0.c1, &ab.c0.c2, &ab.c1.c0, &ab.c1.c1, &ab.c1.c2};
        for (int i = 0; i < 6; ++i) put_fq2(o, *c[i]);
        put_g2_prepared(o, neg(vk.gamma_g2));
        put_g2_prepared(o, neg(vk.delta_g2));
        if (o.size() != need) throw HipError(CG_ERR_HIP, "internal size mismatch");
        memcpy(pvk_out, o.data(), need);
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}
