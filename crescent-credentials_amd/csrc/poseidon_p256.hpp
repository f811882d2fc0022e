// Poseidon over P-256's base field, width 3, and h_Q = `compute_hQ` (ecdsa-pop/src/lib.rs:308-320) on it, written once for
// host and device in the manner of sha256.hpp: tests/cpp/test_poseidon_p256.cpp runs it under plain g++.
//   - the CONSTANTS, as neptune derives them for `Strength::Standard` (ecdsa-pop/neptune/src/round_numbers.rs,
//     round_constants.rs, mds.rs): (R_F, R_P) = (8, 55) for t = 3; 63 x 3 round constants drawn from the Grain LFSR seeded
//     with (field = 1, sbox = 1, field bits, t, R_F, R_P, thirty ones) by rejection sampling; the Cauchy matrix
//     M[i][j] = 1 / (i + j + t).  The host derives them once per process (pos_consts); nothing is stored as a table here.
//     A handle uploads them on first use: POS_N_CONSTS elements in Montgomery form, 6.4 KB.
//   - the PERMUTATION in its plain ("Correct") form: add the round's constants, x^5 on every element in the 4 + 4 full rounds
//     and on element 0 alone in the 55 partial ones, then the matrix.  neptune's default `OptimizedStatic` computes the same
//     function (its `hash_values` asserts so, and the identity does not depend on the field).
//   - h_Q: the sponge of ecdsa-pop/src/poseidon.rs:103-122 over (q0, q1, z), and the bytes it is handed on as.
//
// UNVERIFIED in the sense of DESIGN.md §3: the restatement reproduces neptune's own known answers over BLS12-381's Fr
// (tests/test_poseidon_cpu.py, tests/golden/neptune_kats.json), which pins the round numbers, the LFSR, the matrix, the round
// function and the IO-pattern tag.  Three readings nothing pins, each ONE function here and one in tests/poseidon_vectors.py,
// until a Rust-made h_Q meets this code:
//   1. pos_grain_first_byte_bits: a field element is drawn as 32 bytes big-endian whose first byte takes `bits % 8` bits -
//      or 8 where that is 0 (round_constants.rs:135-146).  P-256's field has 256 bits and is the only user of that branch;
//      BLS12-381's Fr takes 7.
//   2. pos_hq_sponge: `api_constants(Standard)`, arity 2, Simplex, IOPattern[Absorb(3), Squeeze(1)] read through
//      sponge/api.rs:196-245 and sponge/vanilla.rs:177-205,442-455 as: state = [tag, 0, 0]; add q0 and q1 to elements 1 and
//      2, permute; add z to element 1, permute (the padding of `HashType::Sponge` is a no-op); the output is element 1.
//      The tag is the IO pattern's 128-bit hash (sponge/api.rs), which pos_io_tag restates and the known answers pin.
//   3. pos_hq_bytes: `to_bytes()` reversed (lib.rs:317-319) read as the element's 32 bytes BIG-endian, `to_repr()` being
//      little-endian (ecdsa-pop/src/utils.rs:463-467).
//
// The round loop is NOT unrolled: the round index is the same in every lane, so the constants are read at a uniform address
// from global memory, and the state is three elements of eight words each in registers.  No per-lane array is indexed by a
// run-time value, so the kernels built on this declare no private segment.
#pragma once
#include "fp256.hpp"

namespace cg {

constexpr int POS_T = 3;                   // width: arity 2 and the capacity element
constexpr int POS_RF = 8, POS_RP = 55;     // round_numbers.rs for t = 3 at 128 bits of security with the 7.5 % margin
constexpr int POS_ROUNDS = POS_RF + POS_RP;
constexpr int POS_N_RC = POS_ROUNDS * POS_T;
constexpr int POS_FIELD_BITS = 256;
// the table a handle uploads: the round constants, the matrix row-major, the tag of h_Q's IO pattern; Montgomery form
constexpr int POS_MDS = POS_N_RC, POS_TAG = POS_N_RC + POS_T * POS_T, POS_N_CONSTS = POS_TAG + 1;

// ---- the permutation ----------------------------------------------------------------------------------------------------
CG_HD void pos_permute(const F256* __restrict__ c, F256& s0, F256& s1, F256& s2) {
    const F256* m = c + POS_MDS;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (int r = 0; r < POS_ROUNDS; ++r) {
        const F256* k = c + POS_T * r;
        s0 = f256_pow5(f256_add(s0, k[0]));
        s1 = f256_add(s1, k[1]);
        s2 = f256_add(s2, k[2]);
        if (r < POS_RF / 2 || r >= POS_RF / 2 + POS_RP) {
            s1 = f256_pow5(s1);
            s2 = f256_pow5(s2);
        }
        const F256 n0 = f256_add(f256_add(f256_mul(m[0], s0), f256_mul(m[1], s1)), f256_mul(m[2], s2));
        const F256 n1 = f256_add(f256_add(f256_mul(m[3], s0), f256_mul(m[4], s1)), f256_mul(m[5], s2));
        const F256 n2 = f256_add(f256_add(f256_mul(m[6], s0), f256_mul(m[7], s1)), f256_mul(m[8], s2));
        s0 = n0;
        s1 = n1;
        s2 = n2;
    }
}

// one row of cg_poseidon_p256_permute_batch: three canonical elements of eight words in, three out; false (nothing
// written) where an element is not below p
CG_HD bool pos_permute_row(const F256* __restrict__ c, const uint32_t* in, uint32_t* out) {
    if (!f256_below_p(in) || !f256_below_p(in + 8) || !f256_below_p(in + 16)) return false;
    F256 s0 = f256_from_words(in), s1 = f256_from_words(in + 8), s2 = f256_from_words(in + 16);
    pos_permute(c, s0, s1, s2);
    f256_to_words(s0, out);
    f256_to_words(s1, out + 8);
    f256_to_words(s2, out + 16);
    return true;
}

// ---- h_Q ------------------------------------------------------------------------------------------------------------------
// reading 2: the sponge over canonical q0, q1 and z (eight words each, below p) -> element 1 after the second permutation
CG_HD F256 pos_hq_sponge(const F256* __restrict__ c, const uint32_t* q0, const uint32_t* q1, const uint32_t* z) {
    F256 s0 = c[POS_TAG], s1 = f256_from_words(q0), s2 = f256_from_words(q1);
    pos_permute(c, s0, s1, s2);
    s1 = f256_add(s1, f256_from_words(z));
    pos_permute(c, s0, s1, s2);
    return s1;
}
// reading 3: the element's canonical value as 32 bytes big-endian, written as eight words (out is 4-byte aligned)
CG_HD void pos_hq_bytes(const F256& h, uint32_t* out) {
    uint32_t w[8];
    f256_to_words(h, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t x = w[7 - i];
        out[i] = (x << 24) | ((x & 0xff00u) << 8) | ((x >> 8) & 0xff00u) | (x >> 24);
    }
}
// a scalar of BN254 as a showing holds it: eight words below r
CG_HD bool pos_below_r(const uint32_t* w) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) br = (((uint64_t)w[i] - FrP::N[i] - br) >> 32) & 1u;
    return br != 0;
}
// one row of cg_hq_batch: q0, q1 and z as canonical Fr (r < p, so each is a field element) -> h_Q's 32 bytes as eight
// words; false and eight zero words where a scalar is not below r
CG_HD bool pos_hq_row(const F256* __restrict__ c, const uint32_t* q0, const uint32_t* q1, const uint32_t* z, uint32_t* out) {
    if (!pos_below_r(q0) || !pos_below_r(q1) || !pos_below_r(z)) {
#pragma unroll
        for (int i = 0; i < 8; ++i) out[i] = 0;
        return false;
    }
    pos_hq_bytes(pos_hq_sponge(c, q0, q1, z), out);
    return true;
}

// ---- the constants: host functions --------------------------------------------------------------------------------------
// reading 1
inline int pos_grain_first_byte_bits(int field_bits) { return field_bits % 8 ? field_bits % 8 : 8; }

// The Grain LFSR of round_constants.rs: 80 bits, b_{i+80} = b_{i+62} ^ b_{i+51} ^ b_{i+38} ^ b_{i+23} ^ b_{i+13} ^ b_i, the
// first 160 outputs thrown away; a bit is drawn as a pair, kept where the pair's first bit is 1.
struct PosGrain {
    uint8_t st[80];
    int at = 0;                            // st[(at + i) % 80] is b_i
    uint8_t step() {
        auto b = [&](int i) { return st[(at + i) % 80]; };
        const uint8_t n = b(62) ^ b(51) ^ b(38) ^ b(23) ^ b(13) ^ b(0);
        st[at] = n;
        at = (at + 1) % 80;
        return n;
    }
    uint8_t bit() {
        uint8_t first = step();
        while (!first) {
            step();
            first = step();
        }
        return step();
    }
    PosGrain(int field_bits, int t, int rf, int rp) {
        int n = 0;
        auto put = [&](int width, uint32_t v) {
            for (int i = width - 1; i >= 0; --i) st[n++] = (uint8_t)((v >> i) & 1u);
        };
        put(2, 1);                         // a prime field
        put(4, 1);                         // the S-box x^alpha
        put(12, (uint32_t)field_bits);
        put(12, (uint32_t)t);
        put(10, (uint32_t)rf);
        put(10, (uint32_t)rp);
        put(30, 0x3fffffffu);
        for (int i = 0; i < 160; ++i) step();
    }
    // 32 bytes big-endian, the first of them short (reading 1), as eight little-endian words
    void draw(int field_bits, uint32_t w[8]) {
        for (int i = 0; i < 8; ++i) w[i] = 0;
        for (int byte = 0; byte < 32; ++byte) {
            const int bits = byte == 0 ? pos_grain_first_byte_bits(field_bits) : 8;
            uint32_t v = 0;
            for (int i = 0; i < bits; ++i) v = (v << 1) | bit();
            w[(31 - byte) / 4] |= v << (8 * ((31 - byte) % 4));
        }
    }
};

// The tag of an IO pattern (sponge/api.rs): the pattern's words - an absorb of n is n + 2^31, a squeeze of n is n, adjacent
// operations of one kind merged - and the domain separator last, hashed as sum of word_i · x^(i+1) mod 2^128, x = 2^128 - 159.
// For IOPattern[Absorb(3), Squeeze(1)] and separator 0.
inline void pos_io_tag(uint32_t w[8]) {
    typedef unsigned __int128 u128;
    const u128 x = ~(u128)0 - 158;
    const u128 words[3] = {(u128)3 + ((u128)1 << 31), 1, 0};
    u128 xi = 1, sum = 0;
    for (const u128& word : words) {
        xi *= x;
        sum += xi * word;
    }
    for (int i = 0; i < 8; ++i) w[i] = i < 4 ? (uint32_t)(sum >> (32 * i)) : 0u;
}

struct PosConsts {
    F256 c[POS_N_CONSTS];
};
inline PosConsts pos_make_consts() {
    PosConsts k;
    PosGrain g(POS_FIELD_BITS, POS_T, POS_RF, POS_RP);
    uint32_t w[8];
    for (int n = 0; n < POS_N_RC;) {
        g.draw(POS_FIELD_BITS, w);
        if (f256_below_p(w)) k.c[n++] = f256_from_words(w);       // rejection sampling
    }
    for (int i = 0; i < POS_T; ++i)
        for (int j = 0; j < POS_T; ++j) {
            for (int l = 0; l < 8; ++l) w[l] = 0;
            w[0] = (uint32_t)(i + j + POS_T);
            k.c[POS_MDS + POS_T * i + j] = f256_inv(f256_from_words(w));
        }
    pos_io_tag(w);
    k.c[POS_TAG] = f256_from_words(w);
    return k;
}
// once per process
inline const PosConsts& pos_consts() {
    static const PosConsts k = pos_make_consts();
    return k;
}

}  // namespace cg
