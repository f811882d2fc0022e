// The scalar stage of `RangeProof::verify_n_bits` (creds/src/rangeproof.rs:342-424) over Fr: from one proof's evaluations,
// random_v, the two challenges and the caller's two randomizers to what the group stage (csrc/rangeverify.hip) needs
//   - the checks that make a showing CG_VERIFY_MALFORMED: a scalar >= r, rho = 1 or rho = w^(n-1) (the reference divides by
//     rho - 1 and by rho - w^(n-1) and panics at exactly these two values)
//   - the evaluation identity (rangeproof.rs:395-412) and the DLEQ's eq_pos comparison s_00 == s_13 (dlog.rs:155-164)
//   - the scalar of every term of `KZG10::batch_check` (forks/ark-poly-commit/src/kzg10/mod.rs:357-411) with the randomizers
//     r_0 = 1, r_1, r_2 and the coefficients of com_w^ = f_coeff com_f + q_coeff com_q merged in, so that every point
//     is multiplied once:
//       total_c = (1 + r_1) com_g + r_2 f_coeff com_f + r_2 q_coeff com_q + rho W_g + r_1 rho w W_gw + r_2 rho W_w^
//                 - (Σ r_i v_i) g - (Σ r_i random_v_i) gamma_g
//       total_w = W_g + r_1 W_gw + r_2 W_w^
//     Merging scalars does not change the group elements.
// q_coeff = rho^n - 1, f_coeff = q_coeff/(rho - 1); both inverses come from ONE Fermat inversion of (rho - 1)(rho - w^(n-1)).
// A rho with rho^n = 1 other than those two is computed as the reference computes it: q_coeff = f_coeff = 0, com_w^ = O.
//
// Written once for host and device, one lane per showing, as rangepoly.hpp is; tests/cpp/test_rangeverify.cpp runs it under
// plain g++.
#pragma once
#include "rangepoly.hpp"

namespace cg {

// the merged scalars, in the order the group stage lays its terms out: the eight variable-base terms, then the two
// fixed-base ones
enum {
    RV_COM_G = 0,      // 1 + r_1, an integer below 2^129
    RV_COM_F,          // r_2 f_coeff
    RV_COM_Q,          // r_2 q_coeff
    RV_W_G,            // rho
    RV_W_GW,           // r_1 rho w
    RV_W_W,            // r_2 rho
    RV_TW_GW,          // r_1 (total_w), below 2^128
    RV_TW_W,           // r_2 (total_w), below 2^128
    RV_G,              // Σ r_i v_i, subtracted
    RV_GAMMA_G,        // Σ r_i random_v_i, subtracted
    RV_N_SCALARS
};
constexpr int RV_N_VAR_KZG = 8, RV_N_FIX_KZG = 2;
// bits of a variable-base term's scalar: the chain walks no more doublings than that
CG_HD constexpr int rv_scalar_bits(int t) { return t == RV_COM_G ? 129 : (t == RV_TW_GW || t == RV_TW_W) ? 128 : 254; }

enum : uint32_t { RV_MALFORMED = 1u, RV_IDENTITY = 2u, RV_EQ_POS = 4u };

struct RvIn {                 // canonical scalars as the caller passed them
    const uint32_t* evals;    // 3 x 8 words: eval_g, eval_gw, eval_w^
    const uint32_t* proofs;   // 3 x 24 words: W (16) ‖ random_v (8)
    const uint32_t* c;
    const uint32_t* rho;
    const uint32_t* rz;       // 2 x 4 words: r_1, r_2
    const uint32_t* pok_c;    // null: no DLEQ
    const uint32_t* pok_s;    // 6 x 8 words: s_00 s_01 s_10..s_13
};

CG_HD Fr rv_load128(const uint32_t* w) {
    Fr a = Fr::zero();
    for (int i = 0; i < 4; ++i) a.l[i] = w[i];
    return a;
}

// Returns RV_MALFORMED, or the identity and eq_pos bits; the scalars go to out[8 (t stride + l)], canonical, and only for a
// showing that is not malformed.  `stride` is the distance between two terms in scalars (1 on the host; the batch size on
// the device, whose buffers are term-major).
CG_HD uint32_t rv_scalars(const RangeConsts& k, const RvIn& in, uint32_t* out, uint64_t stride) {
    bool ok = rp_below_r(in.c) && rp_below_r(in.rho);
    for (int j = 0; j < 3; ++j) ok = ok && rp_below_r(in.evals + 8 * j) && rp_below_r(in.proofs + 24 * j + 16);
    if (in.pok_c) {
        ok = ok && rp_below_r(in.pok_c);
        for (int j = 0; j < RP_N_RESP; ++j) ok = ok && rp_below_r(in.pok_s + 8 * j);
    }
    if (!ok) return RV_MALFORMED;
    const Fr one = Fr::one();
    const Fr rho = to_mont(rp_load(in.rho)), c = to_mont(rp_load(in.c));
    const Fr a = sub(rho, one), b = sub(rho, k.w_inv);                       // rho - 1, rho - w^(n-1)
    if (a.is_zero() || b.is_zero()) return RV_MALFORMED;
    const Fr iab = inv(mul(a, b));
    const Fr inv_a = mul(iab, b), inv_b = mul(iab, a);
    Fr rho_n = rho;
    for (uint32_t i = 0; i < k.log_n; ++i) rho_n = sqr(rho_n);
    const Fr q_coeff = sub(rho_n, one), f_coeff = mul(q_coeff, inv_a);

    const Fr eg = to_mont(rp_load(in.evals)), egw = to_mont(rp_load(in.evals + 8)), ew = to_mont(rp_load(in.evals + 16));
    // eval_g q_coeff/(rho - 1) + c eval_g (1 - eval_g) q_coeff/(rho - wl) + c^2 d (1 - d)(rho - wl) - eval_w^, d = eval_g - 2 eval_gw
    const Fr w1 = mul(eg, f_coeff);
    const Fr w2 = mul(mul(mul(eg, sub(one, eg)), q_coeff), inv_b);
    const Fr d = sub(eg, dbl(egw));
    const Fr w3 = mul(mul(d, sub(one, d)), b);
    const Fr id = sub(add(add(w1, mul(c, w2)), mul(sqr(c), w3)), ew);
    uint32_t flags = id.is_zero() ? RV_IDENTITY : 0u;
    bool eq = true;
    if (in.pok_c)
        for (int l = 0; l < 8; ++l) eq = eq && in.pok_s[l] == in.pok_s[8 * 5 + l];
    if (eq) flags |= RV_EQ_POS;

    const Fr r1w = rv_load128(in.rz), r2w = rv_load128(in.rz + 4);
    const Fr r1 = to_mont(r1w), r2 = to_mont(r2w);
    auto put = [&](int t, const Fr& canonical) { rp_store(out + 8 * (uint64_t)t * stride, canonical); };
    Fr s = r1w;                                                              // 1 + r_1 as an integer: no reduction, it is below r
    uint32_t carry = 1;
    for (int i = 0; i < 5; ++i) {
        const uint32_t v = s.l[i] + carry;
        carry = v < carry ? 1u : 0u;
        s.l[i] = v;
    }
    put(RV_COM_G, s);
    put(RV_COM_F, from_mont(mul(r2, f_coeff)));
    put(RV_COM_Q, from_mont(mul(r2, q_coeff)));
    put(RV_W_G, rp_load(in.rho));
    put(RV_W_GW, from_mont(mul(r1, mul(rho, k.w))));
    put(RV_W_W, from_mont(mul(r2, rho)));
    put(RV_TW_GW, r1w);
    put(RV_TW_W, r2w);
    put(RV_G, from_mont(add(eg, add(mul(r1, egw), mul(r2, ew)))));
    const Fr v0 = to_mont(rp_load(in.proofs + 16)), v1 = to_mont(rp_load(in.proofs + 40)), v2 = to_mont(rp_load(in.proofs + 64));
    put(RV_GAMMA_G, from_mont(add(v0, add(mul(r1, v1), mul(r2, v2)))));
    return flags;
}

}  // namespace cg

#ifdef __HIPCC__
// ---- the internal entry of rangeverify.hip, for a caller that owns a second handle (cg_verify_showings_batch in verify.hip):
// `verify_n_bits` whole for a chunk of showings whose ped_com is ALREADY ON THE DEVICE and whose verdicts stay there.
// The caller holds the range key's lock for the whole call and orders the range key's stream against its own with events;
// nothing here waits on the host.  The public cg_range_verify_proofs_batch is a thin caller of the same code.
#include "common.hpp"

namespace cg {
std::mutex& range_vk_lock(cg_range_vk* k);
int range_vk_device(const cg_range_vk* k);
hipStream_t range_vk_stream(cg_range_vk* k);
// the 128 bytes registered for `slot`, or null for an unknown slot; under the lock
const uint8_t* range_vk_slot_bytes(const cg_range_vk* k, uint32_t slot);
// room for chunks of `chunk` showings in every per-call array; under the lock, with the key's device current
void range_vk_reserve(cg_range_vk* k, uint64_t chunk);
// rows [off, off + m) of `rows` go up and the kernels of cg_range_verify_proofs_batch are put on the key's stream: ped_com is
// read from d_ped_com (m x 16 words) and the m verdict bytes are written to d_verdicts.  m is at most the chunk reserved.
void range_vk_enqueue(cg_range_vk* k, uint32_t slot, const cg_range_rows& rows, uint64_t off, uint64_t m, const uint32_t* d_ped_com,
                      uint8_t* d_verdicts);
}  // namespace cg
#endif
