// Fixed-base scalar multiplication over 8-bit windows: the geometry of a table, the host code that builds tables of many
// bases with one inversion, and the walk every kernel takes through one (the verifier's x_i·gamma_abc[i+1], a showing's
// responses and nonces, r2·delta_g2 over Fq2, and the setup's six FixedBase::msm calls, generator.rs:140-194).
// Next to it what the same two files share besides: the standard generators, which are the setup's fixed bases and one of
// a key's, and the one variable-base chain of the verifiers' and the showing creator's kernels (scalar_mul_mixed).
// Host and device; builds under plain g++ the way pairing.hpp does (tests/cpp/test_pairing.cpp).
#pragma once
#include <vector>

#include "curve.hpp"

namespace cg {

constexpr int FB_WIN_BITS = 8;
constexpr int FB_WIN = 1 << FB_WIN_BITS;       // entries per window (entry 0 = O)
constexpr int FB_NWIN = 256 / FB_WIN_BITS;     // windows per 256-bit scalar

// fixed-base tables of gabc[1..]: tab[(i·FB_NWIN + w)·FB_WIN + d] = d·2^(8w)·gabc[i+1], affine (one batch inversion).
// The first base is skipped: a verifying key passes gamma_abc_g1 whole, and gamma_abc[0] takes no scalar.
template <class F>
inline void build_tables(const std::vector<Affine<F>>& gabc, std::vector<Affine<F>>& tab) {
    const uint64_t ell = gabc.size() - 1;
    const uint64_t total = ell * FB_NWIN * FB_WIN;
    std::vector<XYZZ<F>> pts(total);
    for (uint64_t i = 0; i < ell; ++i) {
        XYZZ<F> step = XYZZ<F>::from_affine(gabc[i + 1]);
        for (int w = 0; w < FB_NWIN; ++w) {
            XYZZ<F>* row = &pts[(i * FB_NWIN + w) * FB_WIN];
            row[0] = XYZZ<F>::inf();
            for (int d = 1; d < FB_WIN; ++d) {
                row[d] = row[d - 1];
                add(row[d], step);
            }
            XYZZ<F> next = row[FB_WIN - 1];
            add(next, step);
            step = next;
        }
    }
    // batch affine: t_j = zz_j·zzz_j, one inversion of their product
    std::vector<F> pref(total);
    F acc = F::one();
    for (uint64_t j = 0; j < total; ++j) {
        pref[j] = acc;
        if (!pts[j].is_inf()) acc = mul(acc, mul(pts[j].zz, pts[j].zzz));
    }
    F ia = inv(acc);
    tab.resize(total);
    for (uint64_t j = total; j-- > 0;) {
        if (pts[j].is_inf()) { tab[j] = Affine<F>::inf(); continue; }
        const F t = mul(pts[j].zz, pts[j].zzz);
        const F it = mul(ia, pref[j]);          // 1 / t_j
        ia = mul(ia, t);
        tab[j] = {mul(pts[j].x, mul(it, pts[j].zzz)), mul(pts[j].y, mul(it, pts[j].zz))};
    }
}

// k·base from one base's table (FB_NWIN·FB_WIN entries): byte w of k picks the entry of window w, 32 mixed additions at
// the most.  k is any 256-bit integer, not reduced (a table holds d·2^(8w)·base for every byte value).  k may point to
// global memory or, once this is inlined, at the limbs of a value in registers: the byte is taken as k[w >> 2] in both
// cases, which the compiler resolves without scratch.
template <class F>
CG_HD XYZZ<F> fixed_base_mul(const Affine<F>* tab, const uint32_t k[8]) {
    XYZZ<F> acc = XYZZ<F>::inf();
    for (int w = 0; w < FB_NWIN; ++w) {
        const uint32_t d = (k[w >> 2] >> (8 * (w & 3))) & 0xFFu;
        if (d) madd(acc, tab[w * FB_WIN + d]);
    }
    // a copy, not `return acc`: built in place in the caller's result, the accumulator costs k_vfy_inputs and k_mk_fixed
    // ten VGPRs (126 / 127 -> 136) and with them the fourth wave per SIMD
    return XYZZ<F>{acc.x, acc.y, acc.zz, acc.zzz};
}

// k * y for an affine y and k < 2^bits (0 <= bits <= 256): `bits` doublings, each followed by a mixed addition where the bit
// is set, from bit bits - 1 down.  The doublings before the first set bit return at once.  The one variable-base chain of
// the kernels: a length known where it is inlined (the 254 below) costs what a loop written for that length costs.
template <class F>
CG_HD XYZZ<F> scalar_mul_mixed(const Affine<F>& y, const uint32_t* k, int bits) {
    XYZZ<F> acc = XYZZ<F>::inf();
    const int top = (bits - 1) >> 5;
    for (int wi = top; wi >= 0; --wi) {
        const uint32_t kw = k[wi];
        for (int b = wi == top ? (bits - 1) & 31 : 31; b >= 0; --b) {
            acc = dbl(acc);
            if ((kw >> b) & 1u) madd(acc, y);
        }
    }
    return acc;
}
// any canonical scalar: r < 2^254
template <class F>
CG_HD XYZZ<F> scalar_mul_254_mixed(const Affine<F>& y, const uint32_t k[8]) { return scalar_mul_mixed(y, k, 254); }

// The standard generators (ark-bn254 g1.rs, g2.rs; the fork fixes them, generator.rs:34-35), host side, Montgomery form.
// G2's coordinates are parsed from their decimal strings, as ark-bn254's source states them, instead of trusting
// hand-copied limbs.
inline Fq fq_parse_decimal(const char* s) {
    // acc = acc*10 + digit, in Montgomery form
    Fq acc = Fq::zero();
    Fq ten = Fq::zero();
    ten.l[0] = 10;
    ten = to_mont(ten);
    for (const char* p = s; *p; ++p) {
        Fq d = Fq::zero();
        d.l[0] = (uint32_t)(*p - '0');
        acc = add(mul(acc, ten), to_mont(d));
    }
    return acc;
}
inline G1Affine g1_generator() {
    Fq x = Fq::one();
    Fq y = add(Fq::one(), Fq::one());
    return {x, y};
}
inline G2Affine g2_generator() {
    return {{fq_parse_decimal("10857046999023057135944570762232829481370756359578518086990519993285655852781"),
             fq_parse_decimal("11559732032986387107991004021392285783925812861821192530917403151452391805634")},
            {fq_parse_decimal("8495653923123431417604973247489272438418190587263600148770280649306958101930"),
             fq_parse_decimal("4082367875863433681332203403145435568316851327593401208105741076214120093531")}};
}

}  // namespace cg
