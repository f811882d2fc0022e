// The scalar field of P-256 (secp256r1), n = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551, the order of
// the group of csrc/p256.hpp, written once for host and device: the field in which `compute_TU` and `compute_RTU`
// (ecdsa-pop/src/lib.rs:180-240) invert r and s and form the scalars of T, U and R.
//
// The choices are fp256.hpp's, for its reason: n > 2^255, so field.hpp's Fp<P>, which relies on 2N < 2^256, cannot hold it.
// Montgomery form, R = 2^256, eight 32-bit limbs little-endian, always CANONICAL (below n) between operations, and the ninth
// word carried through `add`, `reduce_once` and `mul`.
//
// What the modulus does not give: n has no special shape, so the reduction is the general one.  A round of `mul` adds a·b_i to
// the running value t, takes the quotient digit m = t[0]·(-n^-1 mod 2^32) mod 2^32, adds m·n, which clears word 0, and drops
// that word.  The constant is computed below by Newton's iteration on n's low word, in a constexpr; R^2 mod n is stated, and
// tests/cpp/test_p256.cpp derives both again.
//
// Bounds of `mul` (a, b < n): if t < 2n before a round then t + a·b_i + m·n < 2n + (2^32 - 1)·n + (2^32 - 1)·n = 2^33·n
// < (2 + 2^33)·n < 2^290, and after the division by 2^32 it is below 2n again: eight words and a ninth, `hi`, of at most 1.
// Within the round `hi` collects the carry out of word 7 of t + a·b_i (below 2^32) on top of its own bit, so it is a 64-bit
// variable; the carry chain of the second pass adds it at word 7 and leaves the new ninth bit.  Every step of both chains is
// (2^32 - 1)^2 + 2·(2^32 - 1) = 2^64 - 1 at most, so a 64-bit accumulator holds it.  The result, below 2n with its ninth
// bit in `hi`, takes one conditional subtraction: by n if hi is set or the eight words are not below n.  `add` keeps the
// carry out of limb 7 in the same way; `sub` adds n back after a borrow, and the carry out of that addition cancels the borrow.
#pragma once
#include "field.hpp"

namespace cg {

struct alignas(16) Q256 {
    uint32_t l[8];
};

CG_HD constexpr uint32_t q256_n(int i) {
    constexpr uint32_t n[8] = {0xfc632551u, 0xf3b9cac2u, 0xa7179e84u, 0xbce6faadu, 0xffffffffu, 0xffffffffu, 0x00000000u, 0xffffffffu};
    return n[i];
}
// -n^-1 mod 2^32: x <- x·(2 - n0·x) doubles the number of correct low bits of n0^-1, and x = n0 is right to three bits for
// an odd n0, so five steps give 96 >= 32
CG_HD constexpr uint32_t q256_ninv() {
    const uint32_t n0 = q256_n(0);
    uint32_t x = n0;
    for (int i = 0; i < 5; ++i) x *= 2u - n0 * x;
    return 0u - x;
}
static_assert((uint32_t)(q256_n(0) * q256_ninv()) == 0xffffffffu, "n0 · (-n^-1) = -1 mod 2^32");
// R^2 mod n = 2^512 mod n, which takes a canonical residue into Montgomery form (tests/cpp/test_p256.cpp derives it again by
// 512 doublings of 1)
CG_HD constexpr uint32_t q256_r2(int i) {
    constexpr uint32_t r2[8] = {0xbe79eea2u, 0x83244c95u, 0x49bd6fa6u, 0x4699799cu, 0x2b6bec59u, 0x2845b239u, 0xf3d95620u, 0x66e12d94u};
    return r2[i];
}

CG_HD Q256 q256_zero() {
    Q256 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.l[i] = 0;
    return r;
}
CG_HD bool q256_eq(const Q256& a, const Q256& b) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) o |= a.l[i] ^ b.l[i];
    return o == 0;
}
CG_HD bool q256_is_zero(const Q256& a) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) o |= a.l[i];
    return o == 0;
}

// the eight words at w, as an integer, are below n
CG_HD bool q256_below_n(const uint32_t* w) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) br = (((uint64_t)w[i] - q256_n(i) - br) >> 32) & 1u;
    return br != 0;
}

// a (eight words and the ninth bit `hi`, below 2n as a whole) -> a mod n
CG_HD void q256_reduce_once(uint32_t a[8], uint32_t hi) {
    uint32_t t[8];
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t d = (uint64_t)a[i] - q256_n(i) - br;
        t[i] = (uint32_t)d;
        br = (d >> 32) & 1u;
    }
    // take a - n if the ninth bit is set (then the borrow cancels it) or if there was no borrow
    const uint32_t keep = (hi | (uint32_t)(br ^ 1u)) ? 0u : 0xffffffffu;
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = (a[i] & keep) | (t[i] & ~keep);
}

CG_HD Q256 q256_add(const Q256& a, const Q256& b) {
    Q256 r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        c += (uint64_t)a.l[i] + b.l[i];
        r.l[i] = (uint32_t)c;
        c >>= 32;
    }
    q256_reduce_once(r.l, (uint32_t)c);
    return r;
}

CG_HD Q256 q256_sub(const Q256& a, const Q256& b) {
    Q256 r;
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
        c += (uint64_t)r.l[i] + (q256_n(i) & m);
        r.l[i] = (uint32_t)c;
        c >>= 32;
    }
    return r;
}
CG_HD Q256 q256_neg(const Q256& a) { return q256_sub(q256_zero(), a); }

// Montgomery product a·b·R^-1 mod n of canonical a and b; the header has the bounds
CG_HD Q256 q256_mul(const Q256& a, const Q256& b) {
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
        // t <- (t + m n) / 2^32: word 0 of the sum is zero by the choice of m
        const uint32_t m = t[0] * q256_ninv();
        c = ((uint64_t)m * q256_n(0) + t[0]) >> 32;
#pragma unroll
        for (int j = 1; j < 8; ++j) {
            c += (uint64_t)m * q256_n(j) + t[j];
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        c += hi;
        t[7] = (uint32_t)c;
        hi = c >> 32;                      // 0 or 1: the value is below 2n again
    }
    Q256 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.l[i] = t[i];
    q256_reduce_once(r.l, (uint32_t)hi);
    return r;
}
CG_HD Q256 q256_sqr(const Q256& a) { return q256_mul(a, a); }

CG_HD Q256 q256_to_mont(const Q256& a) {
    Q256 r2;
#pragma unroll
    for (int i = 0; i < 8; ++i) r2.l[i] = q256_r2(i);
    return q256_mul(a, r2);
}
CG_HD Q256 q256_from_mont(const Q256& a) {
    Q256 one = q256_zero();
    one.l[0] = 1;
    return q256_mul(a, one);
}

// any eight words, an integer below 2^256 < 2n, reduced mod n by one conditional subtraction and taken into Montgomery
// form: how the reference's `from_str_vartime` reads R.x and the digest
CG_HD Q256 q256_from_words_reduced(const uint32_t* in) {
    Q256 a;
#pragma unroll
    for (int i = 0; i < 8; ++i) a.l[i] = in[i];
    q256_reduce_once(a.l, 0u);
    return q256_to_mont(a);
}
CG_HD void q256_to_words(const Q256& a, uint32_t* out) {
    const Q256 c = q256_from_mont(a);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = c.l[i];
}

// word w of n, w a run-time value: selected from the eight literals, never indexed out of an array in memory
CG_HD uint32_t q256_n_word(int w) {
    uint32_t e = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) e = w == i ? q256_n(i) : e;
    return e;
}

// a^-1 by Fermat (a != 0; zero gives zero): n - 2 = n with word 0 lowered by 2.  One product site in a rolled loop: on the
// device a lane runs its 512 steps one after the other whatever the code's size, and the kernel stays small.
CG_HD Q256 q256_inv(const Q256& a) {
    Q256 one = q256_zero();
    one.l[0] = 1;
    Q256 r = q256_to_mont(one);
#pragma unroll 1
    for (int s = 0; s < 512; ++s) {
        const int bit = 255 - (s >> 1);
        const uint32_t e = q256_n_word(bit >> 5) - ((bit >> 5) == 0 ? 2u : 0u);
        const bool square = (s & 1) == 0;
        if (!square && !((e >> (bit & 31)) & 1u)) continue;
        r = q256_mul(r, square ? r : a);
    }
    return r;
}

}  // namespace cg
