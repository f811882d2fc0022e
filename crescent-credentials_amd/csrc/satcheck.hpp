// Is one R1CS row satisfied?  <A_i,w>·<B_i,w> = <C_i,w>  (the rule of `ConstraintSystem::is_satisfied` /
// `which_is_unsatisfied`, which the reference runs in forks/circom-compat/src/circom/builder.rs:82-94 and
// forks/groth16/src/prover.rs:197) on the vectors the sparse products leave in HBM (wmap29.hip k_w_to29 / k_sell29).
// Host + device: tests/cpp/test_satcheck.cpp runs the same function under g++ against Python integers.
//
// Operands: a, b, c = 32-byte packed R' form (x·2^261 mod N) as k_sell29 stores it - ANY representative below 2^256
// (k_sell29 leaves values below 3N, k_w_to29 below 2N; 2^256 < 5.3N is what the packed form can hold at all), NOT
// canonical.  Bounds, in the style of field29.hpp (tools/bounds29.py `sat_row` replays them):
//   A, B, C = unpack29(..)      normalised, value < 2^256 < 5.3N, limb 8 < 2^24
//   p = mul(A, B)               normalised, value < A·B/R' + N < (5.3N)²/(169N) + N < 1.17N      [= a·b·R']
//   d = p + 7N - C  (sub<7,1>)  C normalised (T = 1) and < 6N (K - 1 = 6): no limb goes negative; 1.7N < d < 8.17N
//   normalize(d)                limbs 0..7 < 2^29, limb 8 < 2^26: within mul's 2^60 limb-product bound
//   canonical(d)                = cond_sub_n(mul(d, R' mod N)): mul gives d·R'/R' ≡ d with value < 8.17N·N/(169N) + N < 1.05N,
//                               below the 2N cond_sub_n asks for; the result is THE representative in [0, N)
// so the row holds iff every limb of canonical(d) is zero: an exact test, whatever multiples of N the lazy operands carry.
#pragma once
#include "field29.hpp"

namespace cg {

// the canonical value of (a·b - c)·R' mod N; zero iff the row is satisfied
CG_HD Fr29 sat_row_residue(const uint32_t a[8], const uint32_t b[8], const uint32_t c[8]) {
    const Fr29 A = unpack29<Fr29P>(a), B = unpack29<Fr29P>(b), C = unpack29<Fr29P>(c);
    return canonical(normalize(sub<7, 1>(mul(A, B), C)));
}
CG_HD bool sat_row_ok(const uint32_t a[8], const uint32_t b[8], const uint32_t c[8]) { return sat_row_residue(a, b, c).all_zero(); }

// x·R' (packed, any representative below 2^256) -> the plain canonical integer x, eight little-endian words (for the report)
CG_HD void sat_row_value(const uint32_t packed[8], uint32_t out[8]) {
    const Fr x = to_canonical_bytes(unpack29<Fr29P>(packed));      // mul(v, 1) < 5.3N/169 + N < 2N, then cond_sub_n
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = x.l[i];
}

}  // namespace cg
