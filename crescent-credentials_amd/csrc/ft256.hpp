// The base field of T-256 (forks/halo2curves/src/t256/fp.rs:10),
//     p_T = 0x ffffffff00000001 0000000000000001 7e72b42b30e73177 93135661b1c4b117,
// written once for host and device: the field under the group of csrc/t256.hpp, in which every commitment of pi2's Spartan proof lives.
//
// The choices are fq256.hpp's, for its reason: p_T > 2^255, so field.hpp's Fp<P>, which relies on 2N < 2^256, cannot hold it.
// Montgomery form, R = 2^256, eight 32-bit limbs little-endian, always CANONICAL (below p_T) between operations, and the ninth
// word carried through `add`, `reduce_once` and `mul`.  The scheme is restated here and not shared: fq256.hpp and fp256.hpp
// stay as they are, and folding the three onto one template is a refactoring of its own.
//
// p_T has no shape a reduction could use below its top two words, so the reduction is the general one.  A round of `mul` adds
// a·b_i to the running value t, takes the quotient digit m = t[0]·(-p_T^-1 mod 2^32) mod 2^32, adds m·p_T, which clears word 0,
// and drops that word.  The constant (0x0f646959) is computed below by Newton's iteration on p_T's low word, in a constexpr;
// R^2 mod p_T is stated, and tests/cpp/test_t256.cpp derives both again.
//
// Bounds of `mul` (a, b < p_T): if t < 2 p_T before a round then t + a·b_i + m·p_T < 2 p_T + 2 (2^32 - 1) p_T = 2^33 p_T
// < 2^290, and after the division by 2^32 it is below 2 p_T again: eight words and a ninth, `hi`, of at most 1.  Within the
// round `hi` collects the carry out of word 7 of t + a·b_i (below 2^32) on top of its own bit, so it is a 64-bit variable; the
// carry chain of the second pass adds it at word 7 and leaves the new ninth bit.  Every step of both chains is at most
// (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1, so a 64-bit accumulator holds it.  The result, below 2 p_T with its ninth bit in
// `hi`, takes one conditional subtraction: by p_T if hi is set or the eight words are not below p_T.  The last case without
// the first - no ninth bit, yet not below p_T - has room 2^256 - p_T, about 2^224, so random operands meet it once in 2^32:
// tests/test_t256_host.py steers operands to it.  `add` keeps the carry out of limb 7 in the same way; `sub` adds p_T back
// after a borrow, and the carry out of that addition cancels the borrow.
#pragma once
#include "field.hpp"

namespace cg {

struct alignas(16) FT256 {
    uint32_t l[8];
};

CG_HD constexpr uint32_t ft256_p(int i) {
    constexpr uint32_t p[8] = {0xb1c4b117u, 0x93135661u, 0x30e73177u, 0x7e72b42bu, 0x00000001u, 0x00000000u, 0x00000001u, 0xffffffffu};
    return p[i];
}
// -p_T^-1 mod 2^32: x <- x·(2 - p0·x) doubles the number of correct low bits of p0^-1, and x = p0 is right to three bits for
// an odd p0, so five steps give 96 >= 32
CG_HD constexpr uint32_t ft256_pinv() {
    const uint32_t p0 = ft256_p(0);
    uint32_t x = p0;
    for (int i = 0; i < 5; ++i) x *= 2u - p0 * x;
    return 0u - x;
}
static_assert((uint32_t)(ft256_p(0) * ft256_pinv()) == 0xffffffffu, "p0 · (-p_T^-1) = -1 mod 2^32");
// R^2 mod p_T = 2^512 mod p_T, which takes a canonical residue into Montgomery form (tests/cpp/test_t256.cpp derives it again
// by 512 doublings of 1)
CG_HD constexpr uint32_t ft256_r2(int i) {
    constexpr uint32_t r2[8] = {0x910d33ecu, 0xbc7ba9fcu, 0x07eae97fu, 0xd8488344u, 0xa0ed6777u, 0x362b66e6u, 0x21d30291u, 0xa057002au};
    return r2[i];
}

CG_HD FT256 ft256_zero() {
    FT256 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.l[i] = 0;
    return r;
}
CG_HD bool ft256_eq(const FT256& a, const FT256& b) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) o |= a.l[i] ^ b.l[i];
    return o == 0;
}
CG_HD bool ft256_is_zero(const FT256& a) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) o |= a.l[i];
    return o == 0;
}

// the eight words at w, as an integer, are below p_T
CG_HD bool ft256_below_p(const uint32_t* w) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) br = (((uint64_t)w[i] - ft256_p(i) - br) >> 32) & 1u;
    return br != 0;
}

// a (eight words and the ninth bit `hi`, below 2 p_T as a whole) -> a mod p_T
CG_HD void ft256_reduce_once(uint32_t a[8], uint32_t hi) {
    uint32_t t[8];
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t d = (uint64_t)a[i] - ft256_p(i) - br;
        t[i] = (uint32_t)d;
        br = (d >> 32) & 1u;
    }
    // take a - p_T if the ninth bit is set (then the borrow cancels it) or if there was no borrow
    const uint32_t keep = (hi | (uint32_t)(br ^ 1u)) ? 0u : 0xffffffffu;
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = (a[i] & keep) | (t[i] & ~keep);
}

CG_HD FT256 ft256_add(const FT256& a, const FT256& b) {
    FT256 r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        c += (uint64_t)a.l[i] + b.l[i];
        r.l[i] = (uint32_t)c;
        c >>= 32;
    }
    ft256_reduce_once(r.l, (uint32_t)c);
    return r;
}

CG_HD FT256 ft256_sub(const FT256& a, const FT256& b) {
    FT256 r;
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t d = (uint64_t)a.l[i] - b.l[i] - br;
        r.l[i] = (uint32_t)d;
        br = (d >> 32) & 1u;
    }
    const uint32_t m = (uint32_t)0 - (uint32_t)br;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        c += (uint64_t)r.l[i] + (ft256_p(i) & m);
        r.l[i] = (uint32_t)c;
        c >>= 32;
    }
    return r;
}
CG_HD FT256 ft256_neg(const FT256& a) { return ft256_sub(ft256_zero(), a); }

// Montgomery product a·b·R^-1 mod p_T of canonical a and b; the header has the bounds
CG_HD FT256 ft256_mul(const FT256& a, const FT256& b) {
    uint32_t t[8];
    uint64_t hi = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t bi = b.l[i];
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            c += (uint64_t)a.l[j] * bi + t[j];
            t[j] = (uint32_t)c;
            c >>= 32;
        }
        hi += c;
        // t <- (t + m p_T) / 2^32: word 0 of the sum is zero by the choice of m
        const uint32_t m = t[0] * ft256_pinv();
        c = ((uint64_t)m * ft256_p(0) + t[0]) >> 32;
#pragma unroll
        for (int j = 1; j < 8; ++j) {
            c += (uint64_t)m * ft256_p(j) + t[j];
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        c += hi;
        t[7] = (uint32_t)c;
        hi = c >> 32;                      // 0 or 1: the value is below 2 p_T again
    }
    FT256 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.l[i] = t[i];
    ft256_reduce_once(r.l, (uint32_t)hi);
    return r;
}
CG_HD FT256 ft256_sqr(const FT256& a) { return ft256_mul(a, a); }

CG_HD FT256 ft256_to_mont(const FT256& a) {
    FT256 r2;
#pragma unroll
    for (int i = 0; i < 8; ++i) r2.l[i] = ft256_r2(i);
    return ft256_mul(a, r2);
}
CG_HD FT256 ft256_from_mont(const FT256& a) {
    FT256 one = ft256_zero();
    one.l[0] = 1;
    return ft256_mul(a, one);
}

// eight canonical words (below p_T: the caller has checked) -> Montgomery form, and back
CG_HD FT256 ft256_from_words(const uint32_t* in) {
    FT256 a;
#pragma unroll
    for (int i = 0; i < 8; ++i) a.l[i] = in[i];
    return ft256_to_mont(a);
}
CG_HD void ft256_to_words(const FT256& a, uint32_t* out) {
    const FT256 c = ft256_from_mont(a);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = c.l[i];
}

// word w of p_T, w a run-time value: selected from the eight literals, never indexed out of an array in memory
CG_HD uint32_t ft256_p_word(int w) {
    uint32_t e = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) e = w == i ? ft256_p(i) : e;
    return e;
}

// a^-1 by Fermat (a != 0; zero gives zero): p_T - 2 is p_T with word 0 lowered by 2 (its low word ends in 0x17).  One product
// site in a rolled loop: on the device a lane runs its 512 steps one after the other whatever the code's size, and the kernel
// stays small.
CG_HD FT256 ft256_inv(const FT256& a) {
    FT256 one = ft256_zero();
    one.l[0] = 1;
    FT256 r = ft256_to_mont(one);
#pragma unroll 1
    for (int s = 0; s < 512; ++s) {
        const int bit = 255 - (s >> 1);
        const uint32_t e = ft256_p_word(bit >> 5) - ((bit >> 5) == 0 ? 2u : 0u);
        const bool square = (s & 1) == 0;
        if (!square && !((e >> (bit & 31)) & 1u)) continue;
        // the other factor limb by limb: a choice between the two OBJECTS is a choice between two addresses, which would keep
        // the caller's point in memory
        FT256 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o.l[i] = square ? r.l[i] : a.l[i];
        r = ft256_mul(r, o);
    }
    return r;
}

}  // namespace cg
