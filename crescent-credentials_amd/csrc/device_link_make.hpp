// The BN254 half of `DeviceProof::prove` (creds/src/device.rs:104-160) short of `compute_hQ` and pi2: what host and device
// must agree on, written once for both, one lane per proof, as device_link.hpp is for the verifying side;
// tests/cpp/test_device_link_make.cpp runs it under plain g++.
//
// The prover knows every discrete logarithm, so no group element of a proof is a variable-base chain: each is a sum of walks
// through the key's 8-bit tables of g = gamma_abc_g1[pos0 + 1], g' = gamma_abc_g1[pos1 + 1] and h = delta_g1
// (fixed_base.hpp).  Even lhs1 = com0 + e1 com1 + e2 comz - m g is ONE walk: the reference asserts lhs1 == h * r
// (device.rs:153-154), and the opening check below is what makes that hold here.
//   - the terms (one walk each), the sums they form and where the transcripts' points lie in a proof's row of compressed points
//   - the scalar stages: (i) the range checks of the 13 scalars; (ii) pi0's responses after c0; (iii) m and r after the digest;
//     (iv) pi1's responses after c1 - through show_make.hpp's mk_challenge_mont and mk_response_row
//   - the two DLogPoK transcripts, as k_dl_challenge (csrc/devicelink.hip) calls merlin.hpp's ml_dlog_shape_challenge
//   - the opening check: q0 g + r0 h and q1 g' + r1_orig h against the showing's own committed points, in projective form
// The text forms and the digest are device_link.hpp's dl_challenge_digest, with its UNVERIFIED note: no second copy here.
#pragma once
#include "device_link.hpp"
#include "show_make.hpp"

namespace cg {

// ---- the scalars as the caller passes them --------------------------------------------------------------------------------
// openings: `committed_input_openings[1]` and `[2]` of lib.rs:378-379
enum { DLM_Q0 = 0, DLM_R0, DLM_Q1, DLM_R1_ORIG, DLM_N_OPEN };
// rand, in the reference's drawing order: z, t_z (comz); r1 (the re-committed com1); a, b, d (pi0's nonces: r[0] = [a, b],
// r[1] = [a, d], eq_pos (0, 0) applied); n0, n1, n2 (pi1's: r[0] = [n0], r[1] = [n1, n2])
enum { DLM_Z = 0, DLM_TZ, DLM_R1, DLM_A, DLM_B, DLM_D, DLM_N0, DLM_N1, DLM_N2, DLM_N_RAND };

// ---- the group stage ------------------------------------------------------------------------------------------------------
// the walks that depend on no challenge, in the order csrc/devicelinkmake.hip lays their partials out; lhs1 = r h is a
// sixteenth, behind the digest
enum {
    DLM_T_K00_GP = 0,  // a g'          pi0's k_0 = a g' + b h
    DLM_T_K00_H,       // b h
    DLM_T_K01_G,       // a g           pi0's k_1 = a g + d h
    DLM_T_K01_H,       // d h
    DLM_T_K10_H,       // n0 h          pi1's k_0
    DLM_T_K11_G,       // n1 g          pi1's k_1 = n1 g + n2 h
    DLM_T_K11_H,       // n2 h
    DLM_T_COM1_G,      // q1 g          com1 = q1 g + r1 h
    DLM_T_COM1_H,      // r1 h
    DLM_T_COMZ_G,      // z g           comz = z g + t_z h
    DLM_T_COMZ_H,      // t_z h
    DLM_T_OPEN0_G,     // q0 g          against com0
    DLM_T_OPEN0_H,     // r0 h
    DLM_T_OPEN1_GP,    // q1 g'         against com1_orig
    DLM_T_OPEN1_H,     // r1_orig h
    DLM_N_TERMS
};
// the sums of those walks
enum { DLM_O_K00 = 0, DLM_O_K01, DLM_O_K10, DLM_O_K11, DLM_O_COM1, DLM_O_COMZ, DLM_O_OPEN0, DLM_O_OPEN1, DLM_N_OUT };
// a proof's row of compressed points, 32 bytes each, as the transcripts take them: pi0 absorbs k = (K00, K01) and
// y = (COM1_ORIG, COM1), pi1 k = (K10, K11) and y = (LHS1, COMZ)
enum { DLM_P_K00 = 0, DLM_P_K01, DLM_P_K10, DLM_P_K11, DLM_P_COM1_ORIG, DLM_P_COM1, DLM_P_LHS1, DLM_P_COMZ, DLM_N_POINTS };

enum { DLM_BASE_G = 0, DLM_BASE_GP, DLM_BASE_H };
struct DlmTerm {
    bool from_rand;            // the scalar is rand[index], else openings[index]
    uint32_t index, base;
};
CG_HD DlmTerm dlm_term(uint32_t t) {
    switch (t) {
        case DLM_T_K00_GP: return DlmTerm{true, DLM_A, DLM_BASE_GP};
        case DLM_T_K00_H: return DlmTerm{true, DLM_B, DLM_BASE_H};
        case DLM_T_K01_G: return DlmTerm{true, DLM_A, DLM_BASE_G};
        case DLM_T_K01_H: return DlmTerm{true, DLM_D, DLM_BASE_H};
        case DLM_T_K10_H: return DlmTerm{true, DLM_N0, DLM_BASE_H};
        case DLM_T_K11_G: return DlmTerm{true, DLM_N1, DLM_BASE_G};
        case DLM_T_K11_H: return DlmTerm{true, DLM_N2, DLM_BASE_H};
        case DLM_T_COM1_G: return DlmTerm{false, DLM_Q1, DLM_BASE_G};
        case DLM_T_COM1_H: return DlmTerm{true, DLM_R1, DLM_BASE_H};
        case DLM_T_COMZ_G: return DlmTerm{true, DLM_Z, DLM_BASE_G};
        case DLM_T_COMZ_H: return DlmTerm{true, DLM_TZ, DLM_BASE_H};
        case DLM_T_OPEN0_G: return DlmTerm{false, DLM_Q0, DLM_BASE_G};
        case DLM_T_OPEN0_H: return DlmTerm{false, DLM_R0, DLM_BASE_H};
        case DLM_T_OPEN1_GP: return DlmTerm{false, DLM_Q1, DLM_BASE_GP};
        default: return DlmTerm{false, DLM_R1_ORIG, DLM_BASE_H};
    }
}
// sum o is the terms [first, first + count): every sum has two walks but pi1's k_0, which has one
CG_HD uint32_t dlm_first_term(uint32_t o) { return o <= DLM_O_K10 ? 2 * o : 2 * o - 1; }
CG_HD uint32_t dlm_term_count(uint32_t o) { return o == DLM_O_K10 ? 1u : 2u; }
// where sum o lies in the row of compressed points (the two opening checks have no place there)
CG_HD uint32_t dlm_point_of(uint32_t o) { return o <= DLM_O_K11 ? o : o == DLM_O_COM1 ? (uint32_t)DLM_P_COM1 : (uint32_t)DLM_P_COMZ; }

// Sum o from its partials, part(t) the walk of term t.  The general `add` throughout: chosen rows make the two walks equal
// (a doubling) or opposite (O), and either may be O itself.
template <class PartFn>
CG_HD G1XYZZ dlm_sum(uint32_t o, PartFn part) {
    const uint32_t first = dlm_first_term(o);
    G1XYZZ acc = part(first);
    if (dlm_term_count(o) == 2) add(acc, part(first + 1));
    return acc;
}

// Does the sum s equal the committed point c (affine, O as Affine::inf())?  In the projective form, x ZZ = X and y ZZZ = Y, so
// the check costs no inversion; O against O is equal.
CG_HD bool dlm_opens(const G1XYZZ& s, const G1Affine& c) {
    if (s.is_inf() || c.is_inf()) return s.is_inf() && c.is_inf();
    return mul(c.x, s.zz) == s.x && mul(c.y, s.zzz) == s.y;
}

// ---- the scalar stages: openings 4 x 8 words, rand 9 x 8 words, canonical little-endian ---------------------------------------
// (i) every one of the 13 scalars is below r
CG_HD bool dlm_in_range(const uint32_t* openings, const uint32_t* rand) {
    bool ok = true;
    for (int j = 0; j < DLM_N_OPEN; ++j) ok = ok && link_below_r(openings + 8 * j);
    for (int j = 0; j < DLM_N_RAND; ++j) ok = ok && link_below_r(rand + 8 * j);
    return ok;
}
// (ii) after c0: pi0_s = [a - c0 q1, b - c0 r1_orig, a - c0 q1, d - c0 r1] (dlog.rs:101-109); s: 4 x 8 words
CG_HD void dlm_pi0_responses(const uint32_t c0[8], const uint32_t* openings, const uint32_t* rand, uint32_t* s) {
    const Fr c = mk_challenge_mont(c0);
    mk_response_row(c, openings + 8 * DLM_Q1, rand + 8 * DLM_A, s);
    mk_response_row(c, openings + 8 * DLM_R1_ORIG, rand + 8 * DLM_B, s + 8);
    for (int l = 0; l < 8; ++l) s[16 + l] = s[l];                  // eq_pos (0, 0): the same nonce and the same secret
    mk_response_row(c, rand + 8 * DLM_R1, rand + 8 * DLM_D, s + 24);
}
// (iii) after the digest e = e1 ‖ e2 (4 words each, both below 2^128): m = q0 + q1 e1 + z e2 and r = r0 + r1 e1 + t_z e2,
// canonical (device.rs:139-152)
CG_HD void dlm_recombine(const uint32_t e[8], const uint32_t* openings, const uint32_t* rand, uint32_t m[8], uint32_t r[8]) {
    const Fr e1 = to_mont(dl_load(e, 4)), e2 = to_mont(dl_load(e + 4, 4));
    const Fr mm = add(add(dl_load(openings + 8 * DLM_Q0, 8), mul(e1, dl_load(openings + 8 * DLM_Q1, 8))), mul(e2, dl_load(rand + 8 * DLM_Z, 8)));
    const Fr rr = add(add(dl_load(openings + 8 * DLM_R0, 8), mul(e1, dl_load(rand + 8 * DLM_R1, 8))), mul(e2, dl_load(rand + 8 * DLM_TZ, 8)));
    for (int l = 0; l < 8; ++l) {
        m[l] = mm.l[l];
        r[l] = rr.l[l];
    }
}
// (iv) after c1: pi1_s = [n0 - c1 r, n1 - c1 z, n2 - c1 t_z]; s: 3 x 8 words
CG_HD void dlm_pi1_responses(const uint32_t c1[8], const uint32_t r[8], const uint32_t* rand, uint32_t* s) {
    const Fr c = mk_challenge_mont(c1);
    mk_response_row(c, r, rand + 8 * DLM_N0, s);
    mk_response_row(c, rand + 8 * DLM_Z, rand + 8 * DLM_N1, s + 8);
    mk_response_row(c, rand + 8 * DLM_TZ, rand + 8 * DLM_N2, s + 16);
}

// ---- the transcripts ------------------------------------------------------------------------------------------------------
// The challenge of pi0 (which = 0) or pi1 (which = 1) over a proof's row of compressed points; consts as dl_link_consts
// (device_link.hpp) writes them; sponge: ML_STATE bytes, 8-byte aligned, LDS on the device; c: 32 bytes.
CG_HD void dlm_challenge(uint8_t* sponge, const uint8_t* consts, uint32_t which, const uint32_t* points, uint8_t* c) {
    ml_dlog_shape_challenge(sponge, consts + DL_CTX_LEN * which, DL_CTX_LEN, 2u, [=](uint32_t i) { return which == 1 && i == 0 ? 1u : 2u; },
                            consts + 2 * DL_CTX_LEN + 32 * which, (const uint8_t*)(points + 8 * (DLM_P_K00 + 2 * which)),
                            (const uint8_t*)(points + 8 * (DLM_P_COM1_ORIG + 2 * which)), c);
}

}  // namespace cg
