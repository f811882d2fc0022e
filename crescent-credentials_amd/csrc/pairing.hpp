// BN254 optimal-ate pairing, written once for the host and the device (over field.hpp / curve.hpp): the Fq6 / Fq12
// tower, the ark-ec `bn` G2 line steps, the multi-Miller loop over prepared (or on-the-fly) line coefficients and the
// final exponentiation - what `Groth16::verify_with_processed_vk` (forks/groth16/src/verifier.rs:25-65) and
// `prepare_verifying_key` (verifier.rs:13-20) run.  The statement order of every step is that of ark-ec 0.4
// `models/bn` [ark-mem] as oracle/ark_files.py restates it (g2_prepare, multi_miller_loop, final_exponentiation), so the
// Miller-loop value and the pairing value are byte-identical to ark's, not only equal up to a power: the committed
// `alpha_g1_beta_g2` of every PreparedVerifyingKey was made with ark's exponent.
//
// Tower:  Fq2 = Fq[u]/(u^2 + 1),  Fq6 = Fq2[v]/(v^3 - xi),  Fq12 = Fq6[w]/(w^2 - v),  xi = 9 + u.
// Every value is in Montgomery form.  The host test (tests/cpp/test_pairing.cpp) is a g++ build of this header.
#pragma once
#include "curve.hpp"

#if defined(__HIPCC__)
#define CG_PF __host__ __device__ inline
#else
#define CG_PF inline
#endif

namespace cg {

// ---- constants (Montgomery limbs; derived by tools/pairing_consts.py) --------------------------------------------------
struct PairingConsts {
    // Fq6 Frobenius: c1 *= xi^((q^k-1)/3), c2 *= xi^(2(q^k-1)/3);  Fq12: c1 *= xi^((q^k-1)/6)      (k = 1, 2, 3)
    static constexpr uint32_t FROB6_C1_1[2][8] = {{0x4563ab30u, 0xb5773b10u, 0xa9aa6454u, 0x347f91c8u, 0x242e0991u, 0x7a007127u, 0x118214ecu, 0x1956bcd8u}, {0xa0aa4757u, 0x6e849f1eu, 0x89f89141u, 0xaa1c7b6du, 0xfae0ca3au, 0xb6e713cdu, 0x4e82ebc3u, 0x26694fbbu}};
    static constexpr uint32_t FROB6_C2_1[2][8] = {{0x843abe92u, 0x7361d77fu, 0x273411fbu, 0xa5bb2bd3u, 0x4b3e2399u, 0x9c941f31u, 0xbb9fd3ecu, 0x15df9cddu}, {0x4bd8c949u, 0x5dddfd15u, 0xa4445b60u, 0x62cb29a5u, 0x0c7dd2b9u, 0x37bc870au, 0x3171f0fdu, 0x24830a9du}};
    static constexpr uint32_t FROB12_C1_1[2][8] = {{0x33144907u, 0xaf9ba696u, 0x87afb78au, 0xca6b1d73u, 0xf08a2087u, 0x11bded5eu, 0x1a1f3a7cu, 0x02f34d75u}, {0x4c492d72u, 0xa222ae23u, 0x565de15bu, 0xd00f02a4u, 0x53dfc926u, 0xdc2ff3a2u, 0xb3899551u, 0x10a75716u}};
    static constexpr uint32_t FROB6_C1_2[2][8] = {{0x13e80b9cu, 0x3350c88eu, 0xdb5e56b9u, 0x7dce557cu, 0xb615564au, 0x6001b4b8u, 0x020217e0u, 0x2682e617u}, {0, 0, 0, 0, 0, 0, 0, 0}};
    static constexpr uint32_t FROB6_C2_2[2][8] = {{0xd782e155u, 0x71930c11u, 0xffbe3323u, 0xa6bb947cu, 0xd4741444u, 0xaa303344u, 0x26594943u, 0x2c3b3f0du}, {0, 0, 0, 0, 0, 0, 0, 0}};
    static constexpr uint32_t FROB12_C1_2[2][8] = {{0x00fa1bf2u, 0xca8d8005u, 0x68b39769u, 0xf0c5d614u, 0xad0d4418u, 0x0e201271u, 0xbad856e6u, 0x04290f65u}, {0, 0, 0, 0, 0, 0, 0, 0}};
    static constexpr uint32_t FROB6_C1_3[2][8] = {{0x16ad6badu, 0xc9af22f7u, 0x4aa662b2u, 0xb311782au, 0xe248c7f4u, 0x19eeaf64u, 0xe3439f82u, 0x20273e77u}, {0xf7ce93acu, 0xacc02860u, 0x7ba76b4cu, 0x3933d581u, 0x446c8467u, 0x69e6188bu, 0x4417cc55u, 0x0a46036du}};
    static constexpr uint32_t FROB6_C2_3[2][8] = {{0x7b6762dfu, 0x448a93a5u, 0x28fdeadfu, 0xbfd62df5u, 0x0e9bd47au, 0xd858f5d0u, 0x3476ec58u, 0x06b03d4du}, {0xbcc936d1u, 0x2b19daf4u, 0x56f4299fu, 0xa1a54e7au, 0x5adeaef1u, 0xb533eee0u, 0x84dda0b2u, 0x170c812bu}};
    static constexpr uint32_t FROB12_C1_3[2][8] = {{0x4e46d97du, 0x36531618u, 0xd4c96d9fu, 0x0af7129eu, 0xca1009b5u, 0x659da72fu, 0x83a20d23u, 0x08116d89u}, {0xc39c1939u, 0xb1df4af7u, 0x8a73bf7fu, 0x3d9f0287u, 0x8caf0ae0u, 0x9b222092u, 0xeff054a6u, 0x26684515u}};
    // ark-ec bn::g2::mul_by_char: x *= xi^((q-1)/3), y *= xi^((q-1)/2) after conjugation
    static constexpr uint32_t TWIST_MUL_BY_Q_Y[2][8] = {{0x2936b629u, 0xe4bbdd0cu, 0xe133bacbu, 0xbb30f162u, 0xf9645366u, 0x31a9d1b6u, 0xa500f8ddu, 0x253570beu}, {0x5ffe77c7u, 0xa1d77ce4u, 0x7826d1dbu, 0x07affd11u, 0xbb7edc6bu, 0x6d16bd27u, 0x85defeccu, 0x2c872002u}};
    // b' = 3 / (9 + u) of the twist y^2 = x^3 + b'
    static constexpr uint32_t TWIST_B[2][8] = {{0x77b802a8u, 0x3bf938e3u, 0x3633535du, 0x020b1b27u, 0x49755260u, 0x26b7edf0u, 0x4384a86du, 0x2514c632u}, {0xd1dcff67u, 0x38e7ecccu, 0x93ce0d3eu, 0x65f0b37du, 0x22ac00aau, 0xd749d0ddu, 0x4a688d4du, 0x0141b9ceu}};
    static constexpr uint32_t TWO_INV[8] = {0x4f060572u, 0x87bee7d2u, 0x2f1c6ae5u, 0xd0fd2addu, 0xfcfd4f44u, 0x8f5f7492u, 0x3d9cbfacu, 0x1f37631au};
    // ATE_LOOP_COUNT = 6x + 2 in signed binary (ark-bn254 Config): digit i (0..63) is +1 / -1 where bit i of POS / NEG is
    // set; digit 64 is 1.  25 non-zero digits below the top: 64 doubling + 25 addition + 2 final lines = 91 coefficients.
    static constexpr uint64_t ATE_POS = 0xa1818041c0864428ull;
    static constexpr uint64_t ATE_NEG = 0x0408100802100880ull;
    static constexpr int ATE_TOP = 64;
    static constexpr int N_COEFFS = 91;
    static constexpr uint64_t BN_X = 4965661367192848881ull;     // x > 0 for BN254 (X_IS_NEGATIVE = false)
};

CG_PF Fq fq_const(const uint32_t c[8]) {
    Fq r;
    for (int i = 0; i < 8; ++i) r.l[i] = c[i];
    return r;
}
CG_PF Fq2 fq2_const(const uint32_t c[2][8]) { return {fq_const(c[0]), fq_const(c[1])}; }

// ---- Fq2 helpers ---------------------------------------------------------------------------------------------------
CG_PF Fq2 conj(const Fq2& a) { return {a.c0, neg(a.c1)}; }
CG_PF Fq2 mul_by_fq(const Fq2& a, const Fq& b) { return {mul(a.c0, b), mul(a.c1, b)}; }
// a * xi, xi = 9 + u:  (9 a0 - a1) + (a0 + 9 a1) u
CG_PF Fq2 mul_by_xi(const Fq2& a) {
    Fq t0 = dbl(dbl(dbl(a.c0)));
    Fq t1 = dbl(dbl(dbl(a.c1)));
    return {sub(add(t0, a.c0), a.c1), add(add(t1, a.c1), a.c0)};
}
CG_PF Fq2 frob(const Fq2& a, int k) { return (k & 1) ? conj(a) : a; }

// ---- Fq6 = Fq2[v]/(v^3 - xi) ---------------------------------------------------------------------------------------
struct alignas(16) Fq6 {
    Fq2 c0, c1, c2;
    CG_HD static Fq6 zero() { return {Fq2::zero(), Fq2::zero(), Fq2::zero()}; }
    CG_HD static Fq6 one() { return {Fq2::one(), Fq2::zero(), Fq2::zero()}; }
    CG_HD bool is_zero() const { return c0.is_zero() && c1.is_zero() && c2.is_zero(); }
    CG_HD bool operator==(const Fq6& b) const { return c0 == b.c0 && c1 == b.c1 && c2 == b.c2; }
};
CG_PF Fq6 add(const Fq6& a, const Fq6& b) { return {add(a.c0, b.c0), add(a.c1, b.c1), add(a.c2, b.c2)}; }
CG_PF Fq6 sub(const Fq6& a, const Fq6& b) { return {sub(a.c0, b.c0), sub(a.c1, b.c1), sub(a.c2, b.c2)}; }
CG_PF Fq6 neg(const Fq6& a) { return {neg(a.c0), neg(a.c1), neg(a.c2)}; }
CG_PF Fq6 dbl(const Fq6& a) { return {dbl(a.c0), dbl(a.c1), dbl(a.c2)}; }
// a * v:  (xi a2) + a0 v + a1 v^2
CG_PF Fq6 mul_by_v(const Fq6& a) { return {mul_by_xi(a.c2), a.c0, a.c1}; }
CG_PF Fq6 mul(const Fq6& a, const Fq6& b) {      // Karatsuba, 6 Fq2 products
    Fq2 v0 = mul(a.c0, b.c0), v1 = mul(a.c1, b.c1), v2 = mul(a.c2, b.c2);
    Fq2 t0 = sub(sub(mul(add(a.c1, a.c2), add(b.c1, b.c2)), v1), v2);    // a1 b2 + a2 b1
    Fq2 t1 = sub(sub(mul(add(a.c0, a.c1), add(b.c0, b.c1)), v0), v1);    // a0 b1 + a1 b0
    Fq2 t2 = sub(sub(mul(add(a.c0, a.c2), add(b.c0, b.c2)), v0), v2);    // a0 b2 + a2 b0
    return {add(v0, mul_by_xi(t0)), add(t1, mul_by_xi(v2)), add(t2, v1)};
}
CG_PF Fq6 sqr(const Fq6& a) {                      // CH-SQR2
    Fq2 s0 = sqr(a.c0);
    Fq2 s1 = dbl(mul(a.c0, a.c1));
    Fq2 s2 = sqr(add(sub(a.c0, a.c1), a.c2));
    Fq2 s3 = dbl(mul(a.c1, a.c2));
    Fq2 s4 = sqr(a.c2);
    return {add(s0, mul_by_xi(s3)), add(s1, mul_by_xi(s4)), sub(sub(add(add(s1, s2), s3), s0), s4)};
}
// a * (b0 + b1 v)
CG_PF Fq6 mul_by_01(const Fq6& a, const Fq2& b0, const Fq2& b1) {
    Fq2 v0 = mul(a.c0, b0), v1 = mul(a.c1, b1);
    Fq2 a2b1 = sub(mul(add(a.c1, a.c2), b1), v1);
    Fq2 c1 = sub(sub(mul(add(a.c0, a.c1), add(b0, b1)), v0), v1);
    Fq2 a2b0 = sub(mul(add(a.c0, a.c2), b0), v0);
    return {add(v0, mul_by_xi(a2b1)), c1, add(a2b0, v1)};
}
CG_PF Fq6 mul_by_fq2(const Fq6& a, const Fq2& b) { return {mul(a.c0, b), mul(a.c1, b), mul(a.c2, b)}; }
CG_PF Fq6 inv(const Fq6& a) {
    Fq2 t0 = sub(sqr(a.c0), mul_by_xi(mul(a.c1, a.c2)));
    Fq2 t1 = sub(mul_by_xi(sqr(a.c2)), mul(a.c0, a.c1));
    Fq2 t2 = sub(sqr(a.c1), mul(a.c0, a.c2));
    Fq2 d = add(mul(a.c0, t0), mul_by_xi(add(mul(a.c2, t1), mul(a.c1, t2))));
    Fq2 di = inv(d);
    return {mul(t0, di), mul(t1, di), mul(t2, di)};
}
CG_PF Fq6 frob(const Fq6& a, int k) {
    typedef PairingConsts K;
    Fq6 r = {frob(a.c0, k), frob(a.c1, k), frob(a.c2, k)};
    if (k == 1) { r.c1 = mul(r.c1, fq2_const(K::FROB6_C1_1)); r.c2 = mul(r.c2, fq2_const(K::FROB6_C2_1)); }
    else if (k == 2) { r.c1 = mul_by_fq(r.c1, fq_const(K::FROB6_C1_2[0])); r.c2 = mul_by_fq(r.c2, fq_const(K::FROB6_C2_2[0])); }
    else { r.c1 = mul(r.c1, fq2_const(K::FROB6_C1_3)); r.c2 = mul(r.c2, fq2_const(K::FROB6_C2_3)); }
    return r;
}

// ---- Fq12 = Fq6[w]/(w^2 - v) ---------------------------------------------------------------------------------------
// ark-serialize order of the 384 bytes: c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2 (Fq2 each: c0 ‖ c1)
struct alignas(16) Fq12 {
    Fq6 c0, c1;
    CG_HD static Fq12 one() { return {Fq6::one(), Fq6::zero()}; }
    CG_HD bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
    CG_HD bool operator==(const Fq12& b) const { return c0 == b.c0 && c1 == b.c1; }
};
CG_PF Fq12 mul(const Fq12& a, const Fq12& b) {     // Karatsuba, 3 Fq6 products
    Fq6 v0 = mul(a.c0, b.c0), v1 = mul(a.c1, b.c1);
    Fq6 c1 = sub(sub(mul(add(a.c0, a.c1), add(b.c0, b.c1)), v0), v1);
    return {add(v0, mul_by_v(v1)), c1};
}
CG_PF Fq12 sqr(const Fq12& a) {                    // complex squaring, 2 Fq6 products
    Fq6 ab = mul(a.c0, a.c1);
    Fq6 t = mul(add(a.c0, a.c1), add(a.c0, mul_by_v(a.c1)));
    return {sub(sub(t, ab), mul_by_v(ab)), dbl(ab)};
}
CG_PF Fq12 conj(const Fq12& a) { return {a.c0, neg(a.c1)}; }      // = a^(q^6); the inverse on the cyclotomic subgroup
CG_PF Fq12 inv(const Fq12& a) {
    Fq6 d = inv(sub(sqr(a.c0), mul_by_v(sqr(a.c1))));
    return {mul(a.c0, d), neg(mul(a.c1, d))};
}
CG_PF Fq12 frob(const Fq12& a, int k) {
    typedef PairingConsts K;
    Fq6 c0 = frob(a.c0, k), c1 = frob(a.c1, k);
    if (k == 1) c1 = mul_by_fq2(c1, fq2_const(K::FROB12_C1_1));
    else if (k == 2) c1 = {mul_by_fq(c1.c0, fq_const(K::FROB12_C1_2[0])), mul_by_fq(c1.c1, fq_const(K::FROB12_C1_2[0])),
                           mul_by_fq(c1.c2, fq_const(K::FROB12_C1_2[0]))};
    else c1 = mul_by_fq2(c1, fq2_const(K::FROB12_C1_3));
    return {c0, c1};
}
// f * (c0 + c3 w + c4 v w), ark Fp12::mul_by_034
CG_PF Fq12 mul_by_034(const Fq12& f, const Fq2& c0, const Fq2& c3, const Fq2& c4) {
    Fq6 a = mul_by_fq2(f.c0, c0);
    Fq6 b = mul_by_01(f.c1, c3, c4);
    Fq6 e = mul_by_01(add(f.c0, f.c1), add(c0, c3), c4);
    return {add(mul_by_v(b), a), sub(e, add(a, b))};
}
// squaring in the cyclotomic subgroup (Granger-Scott), ark Fp12::cyclotomic_square
CG_PF void fq4_sqr(const Fq2& a, const Fq2& b, Fq2& t0, Fq2& t1) {   // (a + b y)^2, y^2 = xi
    Fq2 tmp = mul(a, b);
    t0 = sub(sub(mul(add(a, b), add(mul_by_xi(b), a)), tmp), mul_by_xi(tmp));
    t1 = dbl(tmp);
}
CG_PF Fq12 cyclotomic_sqr(const Fq12& f) {
    const Fq2 &r0 = f.c0.c0, &r4 = f.c0.c1, &r3 = f.c0.c2, &r2 = f.c1.c0, &r1 = f.c1.c1, &r5 = f.c1.c2;
    Fq2 t0, t1, t2, t3, t4, t5;
    fq4_sqr(r0, r1, t0, t1);
    fq4_sqr(r2, r3, t2, t3);
    fq4_sqr(r4, r5, t4, t5);
    Fq12 o;
    Fq2 z;
    z = dbl(sub(t0, r0)); o.c0.c0 = add(z, t0);              // 3 t0 - 2 z0
    z = dbl(add(t1, r1)); o.c1.c1 = add(z, t1);              // 3 t1 + 2 z1
    Fq2 xt5 = mul_by_xi(t5);
    z = dbl(add(r2, xt5)); o.c1.c0 = add(z, xt5);            // 3 xi t5 + 2 z2
    z = dbl(sub(t4, r3)); o.c0.c2 = add(z, t4);              // 3 t4 - 2 z3
    z = dbl(sub(t2, r4)); o.c0.c1 = add(z, t2);              // 3 t2 - 2 z4
    z = dbl(add(r5, t3)); o.c1.c2 = add(z, t3);              // 3 t3 + 2 z5
    return o;
}
// f^x on the cyclotomic subgroup, x = BN_X, square-and-multiply from the top bit
CG_PF Fq12 cyclotomic_exp_x(const Fq12& f) {
    Fq12 r = f;
    for (int b = 61; b >= 0; --b) {                 // BN_X < 2^63, bit 62 is its top bit
        r = cyclotomic_sqr(r);
        if ((PairingConsts::BN_X >> b) & 1u) r = mul(r, f);
    }
    return r;
}
// ark-ec Bn::exp_by_neg_x: f^x, then inverted because x is positive for BN254
CG_PF Fq12 exp_by_neg_x(const Fq12& f) { return conj(cyclotomic_exp_x(f)); }

// ark-ec Bn::final_exponentiation.  Returns false for f = 0 (ark's `None`: f.inverse() fails), which rejects.
CG_PF bool final_exponentiation(const Fq12& f, Fq12& out) {
    if (f.is_zero()) return false;
    // easy part f^((q^6 - 1)(q^2 + 1))
    Fq12 f1 = conj(f);
    Fq12 f2 = inv(f);
    Fq12 r = mul(f1, f2);
    f2 = r;
    r = frob(r, 2);
    r = mul(r, f2);
    // hard part (Fuentes-Castaneda et al.): r^(2x(6x^2 + 3x + 1)(q^4 - q^2 + 1)/r)
    Fq12 y0 = exp_by_neg_x(r);
    Fq12 y1 = cyclotomic_sqr(y0);
    Fq12 y2 = cyclotomic_sqr(y1);
    Fq12 y3 = mul(y2, y1);
    Fq12 y4 = exp_by_neg_x(y3);
    Fq12 y5 = cyclotomic_sqr(y4);
    Fq12 y6 = exp_by_neg_x(y5);
    y3 = conj(y3);
    y6 = conj(y6);
    Fq12 y7 = mul(y6, y4);
    Fq12 y8 = mul(y7, y3);
    Fq12 y9 = mul(y8, y1);
    Fq12 y10 = mul(y8, y4);
    Fq12 y11 = mul(y10, r);
    Fq12 y12 = frob(y9, 1);
    Fq12 y13 = mul(y12, y11);
    y8 = frob(y8, 2);
    Fq12 y14 = mul(y8, y13);
    r = conj(r);
    Fq12 y15 = frob(mul(r, y9), 3);
    out = mul(y15, y14);
    return true;
}

// ---- G2 line steps (ark-ec bn::G2Prepared, homogeneous projective, D-type twist) -----------------------------------
struct alignas(16) EllCoeff {
    Fq2 c0, c1, c2;
};
struct alignas(16) G2Proj {
    Fq2 x, y, z;
};
CG_PF EllCoeff line_double(G2Proj& r) {
    const Fq two_inv = fq_const(PairingConsts::TWO_INV);
    Fq2 a = mul_by_fq(mul(r.x, r.y), two_inv);
    Fq2 b = sqr(r.y);
    Fq2 c = sqr(r.z);
    Fq2 e = mul(fq2_const(PairingConsts::TWIST_B), add(dbl(c), c));
    Fq2 f = add(dbl(e), e);
    Fq2 g = mul_by_fq(add(b, f), two_inv);
    Fq2 h = sub(sqr(add(r.y, r.z)), add(b, c));
    Fq2 i = sub(e, b);
    Fq2 j = sqr(r.x);
    Fq2 e_sq = sqr(e);
    r.x = mul(a, sub(b, f));
    r.y = sub(sqr(g), add(dbl(e_sq), e_sq));
    r.z = mul(b, h);
    return {neg(h), add(dbl(j), j), i};
}
CG_PF EllCoeff line_add(G2Proj& r, const G2Affine& q) {
    Fq2 theta = sub(r.y, mul(q.y, r.z));
    Fq2 lambda = sub(r.x, mul(q.x, r.z));
    Fq2 c = sqr(theta);
    Fq2 d = sqr(lambda);
    Fq2 e = mul(lambda, d);
    Fq2 f = mul(r.z, c);
    Fq2 g = mul(r.x, d);
    Fq2 h = sub(add(e, f), dbl(g));
    r.x = mul(lambda, h);
    r.y = sub(mul(theta, sub(g, h)), mul(e, r.y));
    r.z = mul(r.z, e);
    Fq2 j = sub(mul(theta, q.x), mul(lambda, q.y));
    return {lambda, neg(theta), j};
}
// ark-ec bn::g2::mul_by_char: the q-power Frobenius carried to the twist
CG_PF G2Affine mul_by_char(const G2Affine& q) {
    return {mul(conj(q.x), fq2_const(PairingConsts::FROB6_C1_1)), mul(conj(q.y), fq2_const(PairingConsts::TWIST_MUL_BY_Q_Y))};
}
// digit i (0..63) of ATE_LOOP_COUNT: +1, -1 or 0
CG_PF int ate_digit(int i) {
    return ((PairingConsts::ATE_POS >> i) & 1u) ? 1 : ((PairingConsts::ATE_NEG >> i) & 1u) ? -1 : 0;
}
// G2Prepared::from(q) for q != O: the 91 coefficients, in consumption order
CG_PF void g2_prepare(const G2Affine& q, EllCoeff out[PairingConsts::N_COEFFS]) {
    G2Proj r = {q.x, q.y, Fq2::one()};
    const G2Affine nq = {q.x, neg(q.y)};
    int k = 0;
    for (int i = PairingConsts::ATE_TOP - 1; i >= 0; --i) {
        out[k++] = line_double(r);
        const int d = ate_digit(i);
        if (d == 1) out[k++] = line_add(r, q);
        else if (d == -1) out[k++] = line_add(r, nq);
    }
    const G2Affine q1 = mul_by_char(q);
    G2Affine q2 = mul_by_char(q1);
    q2.y = neg(q2.y);
    out[k++] = line_add(r, q1);
    out[k++] = line_add(r, q2);
}

// ark-ec Bn::ell (D-type twist): f *= c0·y_P + (c1·x_P) w + c2 v w
CG_PF Fq12 ell(const Fq12& f, const EllCoeff& c, const G1Affine& p) {
    return mul_by_034(f, mul_by_fq(c.c0, p.y), mul_by_fq(c.c1, p.x), c.c2);
}

// ---- multi-Miller loop over up to three pairs -----------------------------------------------------------------------
// Pairs [0, NF) take their line coefficients from their G2 point on the fly (one coefficient computed per consumption:
// no 91-entry table per proof); pairs [NF, 3) read them from a prepared table of 91.  A pair whose `live` is false (G1
// point = O, or G2Prepared marked infinity) is skipped, as ark's multi_miller_loop filters it out.
struct MillerPairs {
    G1Affine p[3];
    G2Affine q[3];                 // on-the-fly pairs only
    const EllCoeff* tab[3];        // prepared pairs only
    bool live[3];
};
template <int NF>
CG_PF Fq12 multi_miller_loop(const MillerPairs& in) {
    typedef PairingConsts K;
    G2Proj r[NF > 0 ? NF : 1];
#pragma unroll
    for (int j = 0; j < NF; ++j) r[j] = {in.q[j].x, in.q[j].y, Fq2::one()};
    Fq12 f = Fq12::one();
    int k = 0;
    for (int i = K::ATE_TOP; i >= 1; --i) {
        if (i != K::ATE_TOP) f = sqr(f);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (in.live[j]) f = ell(f, j < NF ? line_double(r[j < NF ? j : 0]) : in.tab[j][k], in.p[j]);
        ++k;
        const int d = ate_digit(i - 1);
        if (d != 0) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (in.live[j]) {
                    EllCoeff c;
                    if (j < NF) {
                        const G2Affine qq = {in.q[j].x, d > 0 ? in.q[j].y : neg(in.q[j].y)};
                        c = line_add(r[j < NF ? j : 0], qq);
                    } else {
                        c = in.tab[j][k];
                    }
                    f = ell(f, c, in.p[j]);
                }
            ++k;
        }
    }
#pragma unroll
    for (int step = 0; step < 2; ++step) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (in.live[j]) {
                EllCoeff c;
                if (j < NF) {
                    G2Affine q1 = mul_by_char(in.q[j]);
                    if (step == 1) {
                        q1 = mul_by_char(q1);
                        q1.y = neg(q1.y);
                    }
                    c = line_add(r[j < NF ? j : 0], q1);
                } else {
                    c = in.tab[j][k];
                }
                f = ell(f, c, in.p[j]);
            }
        ++k;
    }
    return f;
}

// ---- group checks (ark's checked deserialisation) and prepare_inputs --------------------------------------------------
CG_PF bool g1_on_curve(const G1Affine& p) {          // y^2 = x^3 + 3 (p != O)
    Fq three = add(dbl(Fq::one()), Fq::one());
    return sqr(p.y) == add(mul(sqr(p.x), p.x), three);
}
CG_PF bool g2_on_twist(const G2Affine& p) {          // y^2 = x^3 + b' (p != O)
    return sqr(p.y) == add(mul(sqr(p.x), p.x), fq2_const(PairingConsts::TWIST_B));
}
CG_PF bool g2_in_subgroup(const G2Affine& p) {       // [r] p = O, p on the twist
    return scalar_mul(G2XYZZ::from_affine(p), FrP::N).is_inf();
}
// verifier.rs:25-39: gamma_abc[0] + Σ x_i·gamma_abc[i+1] (x canonical integers, not Montgomery)
CG_PF G1XYZZ prepare_inputs(const G1Affine* gamma_abc, const Fr* x, int n) {
    G1XYZZ acc = G1XYZZ::from_affine(gamma_abc[0]);
    for (int i = 0; i < n; ++i) add(acc, scalar_mul(G1XYZZ::from_affine(gamma_abc[i + 1]), x[i].l));
    return acc;
}

}  // namespace cg
