// The base field of P-256 (secp256r1), p = 2^256 - 2^224 + 2^192 + 2^96 - 1, written once for host and device: the field
// `compute_hQ` hashes over (ecdsa-pop/src/lib.rs:308-320) and the scalar field of T-256, over which every sumcheck round of
// pi2 runs.
//
// Why not Fp<P> (field.hpp): that template relies on 2N < 2^256 - `add` and `reduce_once` drop the carry out of limb 7 and
// the last step of `mul` throws the ninth word away - and p > 2^255.  Here the ninth word is carried everywhere.
//
// Representation: Montgomery form, R = 2^256, eight 32-bit limbs little-endian, always CANONICAL (below p) between
// operations.  The same 32-bit code runs on the host: it is the reference the GPU tests compare with, not a hot path.
//
// What the prime gives back: p = -1 (mod 2^96), so -p^-1 mod 2^32 = 1 and the Montgomery quotient digit of a round is the
// running value's word 0 itself, m = t[0]; and m·p = m·(p + 1) - m with p + 1 = 2^256 - 2^224 + 2^192 + 2^96, so the round's
// t <- (t + m p) / 2^32 is: drop word 0 (t[0] - m = 0), then add m at words 2, 5 and 7 and subtract it at word 6 of the
// shifted value.  No multiplication by a limb of p anywhere.
//
// Bounds of `mul` (a, b < p): after round i the running value is (a·(b mod 2^32i) + M p) / 2^32i with M < 2^32i, which is
// below a + p < 2p < 2^257: eight words and a ninth, `hi`, of at most 1.  Within a round t + a·b_i + m·p < 2p + 2^33 p <
// 2^290, so `hi` holds up to 34 bits for a moment; it is a 64-bit variable.  The carry of the subtraction at word 6 is
// signed: the chain runs on an int64 whose magnitude stays below 2^35, and it ends non-negative because the whole value is.
// The result, below 2p with its ninth bit in `hi`, takes one conditional subtraction: by p if hi is set or the eight words
// are not below p.  `add` keeps the carry out of limb 7 in the same way; `sub` adds p back after a borrow, and the carry
// out of that addition cancels the borrow.
#pragma once
#include "field.hpp"

// The product is inlined on the device, unlike field.hpp's: a lane of the h_Q kernels runs some 1 600 products one after the
// other and the wave is alone on its SIMD, so the kernel's time is its instruction count.  As a called function it was
// measured slower (k_hq_hash 1.91 ms against 1.70 ms, profiles/device_link_hq.md), although the inlined kernels are 24 000
// instructions each.

namespace cg {

struct alignas(16) F256 {
    uint32_t l[8];
};

CG_HD constexpr uint32_t f256_p(int i) {
    constexpr uint32_t p[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000001u, 0xffffffffu};
    return p[i];
}
// R^2 mod p = 2^512 mod p, which takes a canonical residue into Montgomery form (tests/cpp/test_poseidon_p256.cpp derives
// it again by 512 doublings of 1)
CG_HD constexpr uint32_t f256_r2(int i) {
    constexpr uint32_t r2[8] = {0x00000003u, 0x00000000u, 0xffffffffu, 0xfffffffbu, 0xfffffffeu, 0xffffffffu, 0xfffffffdu, 0x00000004u};
    return r2[i];
}

CG_HD F256 f256_zero() {
    F256 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.l[i] = 0;
    return r;
}
CG_HD bool f256_eq(const F256& a, const F256& b) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) o |= a.l[i] ^ b.l[i];
    return o == 0;
}

// the eight words at w, as an integer, are below p
CG_HD bool f256_below_p(const uint32_t* w) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) br = (((uint64_t)w[i] - f256_p(i) - br) >> 32) & 1u;
    return br != 0;
}

// a (eight words and the ninth bit `hi`, below 2p as a whole) -> a mod p
CG_HD void f256_reduce_once(uint32_t a[8], uint32_t hi) {
    uint32_t t[8];
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t d = (uint64_t)a[i] - f256_p(i) - br;
        t[i] = (uint32_t)d;
        br = (d >> 32) & 1u;
    }
    // take a - p if the ninth bit is set (then the borrow cancels it) or if there was no borrow
    const uint32_t keep = (hi | (uint32_t)(br ^ 1u)) ? 0u : 0xffffffffu;
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = (a[i] & keep) | (t[i] & ~keep);
}

CG_HD F256 f256_add(const F256& a, const F256& b) {
    F256 r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        c += (uint64_t)a.l[i] + b.l[i];
        r.l[i] = (uint32_t)c;
        c >>= 32;
    }
    f256_reduce_once(r.l, (uint32_t)c);
    return r;
}

CG_HD F256 f256_sub(const F256& a, const F256& b) {
    F256 r;
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
        c += (uint64_t)r.l[i] + (f256_p(i) & m);
        r.l[i] = (uint32_t)c;
        c >>= 32;
    }
    return r;
}

// Montgomery product a·b·R^-1 mod p of canonical a and b; the header has the bounds
CG_HD F256 f256_mul(const F256& a, const F256& b) {
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
        // t <- (t + m p) / 2^32 with m = t[0]: word k of the new value is word k + 1 of the old, +m at 2, 5 and 7, -m at 6
        const int64_t m = (int64_t)t[0];
        int64_t s = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            s += (int64_t)t[k + 1];
            if (k == 2 || k == 5) s += m;
            if (k == 6) s -= m;
            t[k] = (uint32_t)s;
            s >>= 32;                      // arithmetic: the carry of the subtraction is -1
        }
        s += (int64_t)hi + m;
        t[7] = (uint32_t)s;
        hi = (uint64_t)(s >> 32);          // 0 or 1: the value is below 2p again
    }
    F256 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.l[i] = t[i];
    f256_reduce_once(r.l, (uint32_t)hi);
    return r;
}
CG_HD F256 f256_sqr(const F256& a) { return f256_mul(a, a); }
// the S-box of Poseidon: three products
CG_HD F256 f256_pow5(const F256& a) {
    const F256 a2 = f256_sqr(a);
    return f256_mul(f256_sqr(a2), a);
}

CG_HD F256 f256_to_mont(const F256& a) {
    F256 r2;
#pragma unroll
    for (int i = 0; i < 8; ++i) r2.l[i] = f256_r2(i);
    return f256_mul(a, r2);
}
CG_HD F256 f256_from_mont(const F256& a) {
    F256 one = f256_zero();
    one.l[0] = 1;
    return f256_mul(a, one);
}

// the canonical 32 bytes little-endian, as eight words: `in` must be below p (f256_below_p)
CG_HD F256 f256_from_words(const uint32_t* in) {
    F256 a;
#pragma unroll
    for (int i = 0; i < 8; ++i) a.l[i] = in[i];
    return f256_to_mont(a);
}
CG_HD void f256_to_words(const F256& a, uint32_t* out) {
    const F256 c = f256_from_mont(a);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = c.l[i];
}

// a^-1 by Fermat (a != 0): the host's, for the Cauchy matrix.  p - 2 = p with word 0 lowered by 2.
inline F256 f256_inv(const F256& a) {
    F256 one = f256_zero();
    one.l[0] = 1;
    F256 r = f256_to_mont(one);
    for (int i = 7; i >= 0; --i)
        for (int b = 31; b >= 0; --b) {
            r = f256_sqr(r);
            const uint32_t e = i == 0 ? f256_p(0) - 2u : f256_p(i);
            if ((e >> b) & 1u) r = f256_mul(r, a);
        }
    return r;
}

// What the group of csrc/p256.hpp needs beyond the above: -a, and an inversion that a device lane can run.  One product site
// in a rolled loop of 512 steps (a square, then a product where the exponent's bit is set), the exponent's word selected
// from the eight literals and never indexed out of an array in memory.  Zero gives zero.
CG_HD F256 f256_neg(const F256& a) { return f256_sub(f256_zero(), a); }
CG_HD F256 f256_inv_hd(const F256& a) {
    F256 one = f256_zero();
    one.l[0] = 1;
    F256 r = f256_to_mont(one);
#pragma unroll 1
    for (int s = 0; s < 512; ++s) {
        const int bit = 255 - (s >> 1), w = bit >> 5;
        uint32_t e = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) e = w == i ? f256_p(i) : e;
        if (w == 0) e -= 2u;
        const bool square = (s & 1) == 0;
        if (!square && !((e >> (bit & 31)) & 1u)) continue;
        r = f256_mul(r, square ? r : a);
    }
    return r;
}

}  // namespace cg
