// The pairing of pairing.hpp for a TEAM of lanes that owns one proof: the latency arrangement of the verifiers.
// pairing.hpp runs a proof's Miller loop and final exponentiation as one lane's dependent chain (about 60 Fq2 products in
// series per Miller step); here the independent Fq2 products of every Fq12 operation run side by side: 12 for a squaring,
// 13 for mul_by_034, 18 for a product, 6 for a cyclotomic squaring.  The results are canonical field elements, so they
// are the bytes pairing.hpp and ark-ec produce whatever the order of the multiplications.
//
// Written once over a lane parameter, as rangepoly.hpp is: `ln.lane`, `ln.nl`, `ln.sync()`.  Every value that one job
// hands to another - the Fq12 accumulator, the products, the G2 point and its line coefficients, the Fq12 registers of
// the final exponentiation - is an Fq2 slot of a team-shared array `sh` (LDS on the device), read with sh.ld(job, slot)
// and written with sh.st(job, slot, v).  A PHASE is a loop of independent jobs strided by ln.nl from ln.lane and ends
// with ln.sync(); a job is normally one Fq2 product with the additions that feed it, and a combine job is additions
// only.  Within a phase no job reads or writes a slot that another job writes: tests/cpp/test_pairing_team.cpp runs
// all of this on one host lane over a shared array that remembers who touched what in which phase and aborts otherwise.
// The `job` argument of ld / st exists for that check alone.
//
// Every branch that encloses a sync() depends only on constants (the ate digits, BN_X) and on values every lane holds
// alike (the live flags, slots read after a sync): the whole team takes it together.
#pragma once
#include "pairing.hpp"

namespace cg {

// ---- the slots of the team-shared array ----------------------------------------------------------------------------
namespace tp {
constexpr int F = 0;                  // the Miller accumulator: c0.c0 c0.c1 c0.c2 c1.c0 c1.c1 c1.c2
constexpr int T = 6;                  // products of the running operation [0, 18), scratch of inv [18, 26)
constexpr int P = 32;                 // G1 point of pair j as one slot {x, y}
constexpr int D = 35;                 // prepared pair j: c0·y_P, c1·x_P of the coefficient in use
constexpr int LN = 41;                // on-the-fly pair j: LSTRIDE slots from LN + j·LSTRIDE
constexpr int LSTRIDE = 26;
constexpr int RB = LN + 3 * LSTRIDE;  // Fq12 registers of the final exponentiation, 6 slots each
constexpr int NREG = 10;
constexpr int SLOTS = RB + 6 * NREG;  // 179 slots, 11.2 KB
// within an on-the-fly pair's slots
enum { RX = 0, RY, RZ, QX, QY, Q1X, Q1Y,
       // line_double: a b c j (y+z)^2 e g^2 e^2          line_add: q.y z, q.x z, theta^2, lambda^2, theta q.x, lambda q.y, ...
       DA = 7, DB, DC, DJ, DHS, DE, DGS, DES,
       AM1 = 7, AM2, AC, AD, AJ1, AJ2, AE, AF, AG, ANX, AT1, AT2, ANZ,
       CO0 = 21, CO3, CO4,            // the step's coefficient, scaled by the G1 point: what mul_by_034 takes
       Q2X = 24, Q2Y };
constexpr int reg(int i) { return RB + 6 * i; }
}  // namespace tp

// the shared array of a build without the race check: the device's (in LDS) and the plain host's
struct TeamMem {
    Fq2 v[tp::SLOTS];
    CG_PF Fq2 ld(int, int slot) const { return v[slot]; }
    CG_PF void st(int, int slot, const Fq2& x) { v[slot] = x; }
};

// one phase: jobs [0, n), then the barrier
template <class L, class FN>
CG_PF void team_phase(L& ln, int n, FN fn) {
    for (int job = ln.lane; job < n; job += ln.nl) fn(job);
    ln.sync();
}

// What one job of a phase does: slot dst = mul ? x·y : x.  The jobs of a phase differ in how they gather x and y and meet
// at ONE product (team_finish): lanes of a wave that reached their products by different branches would run them one
// after the other.
struct TeamJob {
    Fq2 x, y;
    int dst;
    bool mul;
};
template <class S>
CG_PF void team_finish(S& sh, int job, const TeamJob& j) {
    sh.st(job, j.dst, j.mul ? mul(j.x, j.y) : j.x);
}
CG_PF TeamJob team_value(int dst, const Fq2& v) { return {v, v, dst, false}; }
CG_PF TeamJob team_product(int dst, const Fq2& x, const Fq2& y) { return {x, y, dst, true}; }

// a/2: (a + q)/2 for an odd a.  Linear, so it is the halving of the Montgomery form too: the bytes of a·TWO_INV
CG_PF Fq fq_half(const Fq& a) {
    const uint32_t odd = 0u - (a.l[0] & 1u);
    uint32_t t[9];
    uint64_t c = 0;
    for (int i = 0; i < 8; ++i) {
        c += (uint64_t)a.l[i] + (FqP::N[i] & odd);
        t[i] = (uint32_t)c;
        c >>= 32;
    }
    t[8] = (uint32_t)c;
    Fq r;
    for (int i = 0; i < 8; ++i) r.l[i] = (t[i] >> 1) | (t[i + 1] << 31);
    return r;
}
CG_PF Fq2 fq2_half(const Fq2& a) { return {fq_half(a.c0), fq_half(a.c1)}; }
CG_PF Fq2 fq2_of(const Fq& a) { return {a, Fq::zero()}; }          // a·b for b in Fq as an Fq2 product: the same bytes

// ---- Fq6 Karatsuba in pieces: the operands of product k of 6, and component c of the result from the six products ------
template <class GX, class GY>
CG_PF TeamJob kara_prod(int dst, int k, GX x, GY y) {
    const int i0 = k < 3 ? k : (k == 3 ? 1 : 0), i1 = k < 3 ? -1 : (k == 4 ? 1 : 2);
    Fq2 a = x(i0), b = y(i0);
    if (i1 >= 0) {
        a = add(a, x(i1));
        b = add(b, y(i1));
    }
    return team_product(dst, a, b);
}
template <class GP>
CG_PF Fq2 kara_comb(int c, GP p) {
    if (c == 0) return add(p(0), mul_by_xi(sub(sub(p(3), p(1)), p(2))));
    if (c == 1) return add(sub(sub(p(4), p(0)), p(1)), mul_by_xi(p(2)));
    return add(sub(sub(p(5), p(0)), p(2)), p(1));
}
// component c of mul_by_01 from its five products v0 v1 (a1+a2)b1 (a0+a1)(b0+b1) (a0+a2)b0
template <class GP>
CG_PF Fq2 m01_comb(int c, GP p) {
    if (c == 0) return add(p(0), mul_by_xi(sub(p(2), p(1))));
    if (c == 1) return sub(sub(p(3), p(0)), p(1));
    return add(sub(p(4), p(0)), p(1));
}

// ---- the jobs of the Fq12 operations.  `a`, `b`, `o` are the first slots of six; o may be a or b ----------------------
// f^2, 12 products: ab = c0·c1 and t = (c0 + c1)(c0 + v·c1)
template <class S>
CG_PF TeamJob sqr12_prod(S& sh, int job, int lj, int a) {
    const bool t = lj >= 6;
    auto X = [&](int i) { return sh.ld(job, a + i); };
    auto Y = [&](int i) { return sh.ld(job, a + 3 + i); };
    auto S1 = [&](int i) { return t ? add(X(i), Y(i)) : X(i); };
    auto S2 = [&](int i) { return t ? add(X(i), i == 0 ? mul_by_xi(Y(2)) : Y(i - 1)) : Y(i); };
    return kara_prod(tp::T + lj, t ? lj - 6 : lj, S1, S2);
}
template <class S>
CG_PF TeamJob sqr12_comb(S& sh, int job, int lj, int o) {
    auto AB = [&](int k) { return sh.ld(job, tp::T + k); };
    auto TT = [&](int k) { return sh.ld(job, tp::T + 6 + k); };
    Fq2 r;
    if (lj < 3) {
        const Fq2 ab = kara_comb(lj, AB), vab = lj == 0 ? mul_by_xi(kara_comb(2, AB)) : kara_comb(lj - 1, AB);
        r = sub(sub(kara_comb(lj, TT), ab), vab);
    } else {
        r = dbl(kara_comb(lj - 3, AB));
    }
    return team_value(o + lj, r);
}
// a·b, 18 products: c0·c0', c1·c1', (c0 + c1)(c0' + c1')
template <class S>
CG_PF TeamJob mul12_prod(S& sh, int job, int lj, int a, int b) {
    const int g = lj / 6;
    auto X = [&](int i) { return g == 0 ? sh.ld(job, a + i) : g == 1 ? sh.ld(job, a + 3 + i) : add(sh.ld(job, a + i), sh.ld(job, a + 3 + i)); };
    auto Y = [&](int i) { return g == 0 ? sh.ld(job, b + i) : g == 1 ? sh.ld(job, b + 3 + i) : add(sh.ld(job, b + i), sh.ld(job, b + 3 + i)); };
    return kara_prod(tp::T + lj, lj % 6, X, Y);
}
template <class S>
CG_PF TeamJob mul12_comb(S& sh, int job, int lj, int o) {
    auto V0 = [&](int k) { return sh.ld(job, tp::T + k); };
    auto V1 = [&](int k) { return sh.ld(job, tp::T + 6 + k); };
    auto V2 = [&](int k) { return sh.ld(job, tp::T + 12 + k); };
    Fq2 r;
    if (lj < 3) r = add(kara_comb(lj, V0), lj == 0 ? mul_by_xi(kara_comb(2, V1)) : kara_comb(lj - 1, V1));
    else r = sub(sub(kara_comb(lj - 3, V2), kara_comb(lj - 3, V0)), kara_comb(lj - 3, V1));
    return team_value(o + lj, r);
}
// f·(d0 + d3 w + d4 v w), 13 products (Fp12::mul_by_034): f.c0·d0, mul_by_01(f.c1, d3, d4), mul_by_01(f.c0 + f.c1, d0 + d3, d4)
template <class S>
CG_PF TeamJob ell_prod(S& sh, int job, int lj, const Fq2& d0, const Fq2& d3, const Fq2& d4) {
    auto X = [&](int i) { return sh.ld(job, tp::F + i); };
    auto Y = [&](int i) { return sh.ld(job, tp::F + 3 + i); };
    Fq2 x, y;
    if (lj < 3) {
        x = X(lj);
        y = d0;
    } else {
        const int m = (lj - 3) % 5;
        const bool s = lj >= 8;
        auto A = [&](int i) { return s ? add(X(i), Y(i)) : Y(i); };
        const Fq2 b0 = s ? add(d0, d3) : d3;
        if (m == 0) { x = A(0); y = b0; }
        else if (m == 1) { x = A(1); y = d4; }
        else if (m == 2) { x = add(A(1), A(2)); y = d4; }
        else if (m == 3) { x = add(A(0), A(1)); y = add(b0, d4); }
        else { x = add(A(0), A(2)); y = b0; }
    }
    return team_product(tp::T + lj, x, y);
}
template <class S>
CG_PF TeamJob ell_comb(S& sh, int job, int lj) {
    auto B = [&](int k) { return sh.ld(job, tp::T + 3 + k); };
    auto E = [&](int k) { return sh.ld(job, tp::T + 8 + k); };
    Fq2 r;
    if (lj < 3) {
        r = add(lj == 0 ? mul_by_xi(m01_comb(2, B)) : m01_comb(lj - 1, B), sh.ld(job, tp::T + lj));
    } else {
        const int c = lj - 3;
        r = sub(m01_comb(c, E), add(sh.ld(job, tp::T + c), m01_comb(c, B)));
    }
    return team_value(tp::F + lj, r);
}
// cyclotomic squaring, 6 products: (a, b) = (r0, r1), (r2, r3), (r4, r5) as cyclotomic_sqr names them
template <class S>
CG_PF TeamJob cyc_prod(S& sh, int job, int lj, int a) {
    const int p = lj >> 1;
    const Fq2 x = sh.ld(job, a + (p == 0 ? 0 : p == 1 ? 3 : 1)), y = sh.ld(job, a + (p == 0 ? 4 : p == 1 ? 2 : 5));
    return (lj & 1) ? team_product(tp::T + lj, add(x, y), add(mul_by_xi(y), x)) : team_product(tp::T + lj, x, y);
}
template <class S>
CG_PF TeamJob cyc_comb(S& sh, int job, int lj, int a, int o) {
    // t_{2p} = m - tmp - xi tmp, t_{2p+1} = 2 tmp
    auto TE = [&](int p) { const Fq2 tmp = sh.ld(job, tp::T + 2 * p); return sub(sub(sh.ld(job, tp::T + 2 * p + 1), tmp), mul_by_xi(tmp)); };
    auto TO = [&](int p) { return dbl(sh.ld(job, tp::T + 2 * p)); };
    const Fq2 z = sh.ld(job, a + lj);
    Fq2 t;
    bool minus;
    if (lj == 0) { t = TE(0); minus = true; }               // 3 t0 - 2 z0
    else if (lj == 4) { t = TO(0); minus = false; }         // 3 t1 + 2 z1
    else if (lj == 3) { t = mul_by_xi(TO(2)); minus = false; }   // 3 xi t5 + 2 z2
    else if (lj == 2) { t = TE(2); minus = true; }          // 3 t4 - 2 z3
    else if (lj == 1) { t = TE(1); minus = true; }          // 3 t2 - 2 z4
    else { t = TO(1); minus = false; }                      // 3 t3 + 2 z5
    return team_value(o + lj, add(dbl(minus ? sub(t, z) : add(z, t)), t));
}

// ---- whole operations on Fq12 registers: two phases each --------------------------------------------------------------
template <class L, class S>
CG_PF void team_mul12(L& ln, S& sh, int o, int a, int b) {
    team_phase(ln, 18, [&](int job) { team_finish(sh, job, mul12_prod(sh, job, job, a, b)); });
    team_phase(ln, 6, [&](int job) { team_finish(sh, job, mul12_comb(sh, job, job, o)); });
}
template <class L, class S>
CG_PF void team_cyc_sqr(L& ln, S& sh, int o, int a) {
    team_phase(ln, 6, [&](int job) { team_finish(sh, job, cyc_prod(sh, job, job, a)); });
    team_phase(ln, 6, [&](int job) { team_finish(sh, job, cyc_comb(sh, job, job, a, o)); });
}
template <class L, class S>
CG_PF void team_conj(L& ln, S& sh, int o, int a) {
    team_phase(ln, 6, [&](int job) { const Fq2 v = sh.ld(job, a + job); sh.st(job, o + job, job < 3 ? v : neg(v)); });
}
// a^(q^k): each component conjugated for odd k and multiplied by its constants (Fq6's, then Fq12's for c1)
template <class L, class S>
CG_PF void team_frob(L& ln, S& sh, int o, int a, int k) {
    typedef PairingConsts K;
    team_phase(ln, 6, [&](int job) {
        Fq2 v = frob(sh.ld(job, a + job), k);
        const int c = job % 3;
        if (c == 1) v = mul(v, fq2_const(k == 1 ? K::FROB6_C1_1 : k == 2 ? K::FROB6_C1_2 : K::FROB6_C1_3));
        if (c == 2) v = mul(v, fq2_const(k == 1 ? K::FROB6_C2_1 : k == 2 ? K::FROB6_C2_2 : K::FROB6_C2_3));
        if (job >= 3) v = mul(v, fq2_const(k == 1 ? K::FROB12_C1_1 : k == 2 ? K::FROB12_C1_2 : K::FROB12_C1_3));
        sh.st(job, o + job, v);
    });
}
// component c of sqr(Fq6) (CH-SQR2) from x0^2, x0 x1, (x0 - x1 + x2)^2, x1 x2, x2^2
template <class GP>
CG_PF Fq2 sqr6_comb(int c, GP s) {
    if (c == 0) return add(s(0), mul_by_xi(dbl(s(3))));
    if (c == 1) return add(dbl(s(1)), mul_by_xi(s(4)));
    return sub(sub(add(add(dbl(s(1)), s(2)), dbl(s(3))), s(0)), s(4));
}
// 1/a (a != 0).  The Fq inversion inside stays one lane's chain; everything around it is spread.
template <class L, class S>
CG_PF void team_inv12(L& ln, S& sh, int o, int a) {
    constexpr int T = tp::T, U = tp::T + 18, W = tp::T + 21, XI = tp::T + 24;
    team_phase(ln, 10, [&](int job) {                       // sqr(a.c0), sqr(a.c1): five products each
        const int h = job / 5 * 3, m = job % 5;
        auto X = [&](int i) { return sh.ld(job, a + h + i); };
        const Fq2 x = m == 0 ? X(0) : m == 1 ? X(0) : m == 2 ? add(sub(X(0), X(1)), X(2)) : m == 3 ? X(1) : X(2);
        const Fq2 y = m == 1 ? X(1) : m == 3 ? X(2) : x;
        sh.st(job, T + job, mul(x, y));
    });
    team_phase(ln, 3, [&](int job) {                        // d = sqr(a.c0) - v·sqr(a.c1)
        auto SX = [&](int k) { return sh.ld(job, T + k); };
        auto SY = [&](int k) { return sh.ld(job, T + 5 + k); };
        sh.st(job, U + job, sub(sqr6_comb(job, SX), job == 0 ? mul_by_xi(sqr6_comb(2, SY)) : sqr6_comb(job - 1, SY)));
    });
    team_phase(ln, 6, [&](int job) {                        // inv(Fq6) of d: d0^2 d1d2 d2^2 d0d1 d1^2 d0d2
        const int i = job == 0 ? 0 : job == 1 ? 1 : job == 2 ? 2 : job == 3 ? 0 : job == 4 ? 1 : 0;
        const int j = job == 0 ? 0 : job == 1 ? 2 : job == 2 ? 2 : job == 3 ? 1 : job == 4 ? 1 : 2;
        sh.st(job, T + job, mul(sh.ld(job, U + i), sh.ld(job, U + j)));
    });
    team_phase(ln, 3, [&](int job) {
        Fq2 r;
        if (job == 0) r = sub(sh.ld(job, T + 0), mul_by_xi(sh.ld(job, T + 1)));
        else if (job == 1) r = sub(mul_by_xi(sh.ld(job, T + 2)), sh.ld(job, T + 3));
        else r = sub(sh.ld(job, T + 4), sh.ld(job, T + 5));
        sh.st(job, W + job, r);
    });
    team_phase(ln, 3, [&](int job) {                        // d0 t0, d2 t1, d1 t2
        sh.st(job, T + job, mul(sh.ld(job, U + (job == 0 ? 0 : job == 1 ? 2 : 1)), sh.ld(job, W + job)));
    });
    team_phase(ln, 1, [&](int job) {
        sh.st(job, XI, inv(add(sh.ld(job, T + 0), mul_by_xi(add(sh.ld(job, T + 1), sh.ld(job, T + 2))))));
    });
    team_phase(ln, 3, [&](int job) { sh.st(job, U + job, mul(sh.ld(job, W + job), sh.ld(job, XI))); });
    team_phase(ln, 12, [&](int job) {                       // a.c0·d^-1, a.c1·d^-1
        const int h = job / 6 * 3;
        auto X = [&](int i) { return sh.ld(job, a + h + i); };
        auto Y = [&](int i) { return sh.ld(job, U + i); };
        team_finish(sh, job, kara_prod(T + job, job % 6, X, Y));
    });
    team_phase(ln, 6, [&](int job) {
        const int h = job / 3 * 6;
        auto PR = [&](int k) { return sh.ld(job, T + h + k); };
        const Fq2 r = kara_comb(job % 3, PR);
        sh.st(job, o + job, job < 3 ? r : neg(r));
    });
}
// the six slots from `at` as an Fq12 and back: after a sync, by every lane alike (a read) or by lanes [0, 6) (a write)
template <class L, class S>
CG_PF Fq12 team_read12(L& ln, S& sh, int at) {
    Fq12 f;
    f.c0.c0 = sh.ld(ln.lane, at); f.c0.c1 = sh.ld(ln.lane, at + 1); f.c0.c2 = sh.ld(ln.lane, at + 2);
    f.c1.c0 = sh.ld(ln.lane, at + 3); f.c1.c1 = sh.ld(ln.lane, at + 4); f.c1.c2 = sh.ld(ln.lane, at + 5);
    return f;
}
CG_PF const Fq2& fq12_part(const Fq12& f, int i) {
    return i == 0 ? f.c0.c0 : i == 1 ? f.c0.c1 : i == 2 ? f.c0.c2 : i == 3 ? f.c1.c0 : i == 4 ? f.c1.c1 : f.c1.c2;
}
// slots [at, at + 6) == want: every lane reads the same slots, so every lane returns the same answer
template <class L, class S>
CG_PF bool team_equals(L& ln, S& sh, int at, const Fq12& want) {
    bool eq = true;
    for (int i = 0; i < 6; ++i) eq = eq && sh.ld(ln.lane, at + i) == fq12_part(want, i);
    return eq;
}
template <class L, class S>
CG_PF bool team_is_one(L& ln, S& sh, int at) {
    bool eq = sh.ld(ln.lane, at) == Fq2::one();
    for (int i = 1; i < 6; ++i) eq = eq && sh.ld(ln.lane, at + i).is_zero();
    return eq;
}

// ark-ec Bn::final_exponentiation as a program over the Fq12 registers, in final_exponentiation's order and names.  It is
// data, and team_final_exponentiation one loop around one switch, so that the kernel holds the code of each operation
// once (inlined at every use the kernel was 340 KB, several times the instruction cache).
struct FexpProg {
    enum { MUL, CYC, CONJ, FROB, EXPX, INV, COPY };          // o = a·b | a^2 (cyclotomic) | conj a | a^(q^b) | exp_by_neg_x(a), o != a | 1/a
    enum { OUT = 0, R, A, B, Y1, Y3, Y4, Y6, Y8, IN };       // registers
    static constexpr int N = 27;
    static constexpr uint8_t OPS[N][4] = {
        // easy part f^((q^6 - 1)(q^2 + 1))
        {INV, B, IN, 0}, {CONJ, A, IN, 0}, {MUL, R, A, B}, {FROB, A, R, 2}, {MUL, R, A, R},
        // hard part
        {EXPX, A, R, 0},                       // y0
        {CYC, Y1, A, 0},                       // y1
        {CYC, A, Y1, 0},                       // y2
        {MUL, Y3, A, Y1},                      // y3
        {EXPX, Y4, Y3, 0},                     // y4
        {CYC, A, Y4, 0},                       // y5
        {EXPX, Y6, A, 0},                      // y6
        {CONJ, Y3, Y3, 0}, {CONJ, Y6, Y6, 0},
        {MUL, A, Y6, Y4},                      // y7
        {MUL, Y8, A, Y3},                      // y8
        {MUL, Y6, Y8, Y1},                     // y9, in y6's register
        {MUL, A, Y8, Y4},                      // y10
        {MUL, A, A, R},                        // y11
        {FROB, B, Y6, 1},                      // y12
        {MUL, A, B, A},                        // y13
        {FROB, Y8, Y8, 2},
        {MUL, A, Y8, A},                       // y14
        {CONJ, R, R, 0}, {MUL, B, R, Y6}, {FROB, B, B, 3},      // y15
        {MUL, OUT, B, A},
    };
};
// Of register 9 (the caller wrote tp::reg(9) and synced), to register 0.  Returns false for f = 0, on every lane.
template <class L, class S>
CG_PF bool team_final_exponentiation(L& ln, S& sh) {
    typedef FexpProg P;
    bool zero = true;
    for (int i = 0; i < 6; ++i) zero = zero && sh.ld(ln.lane, tp::reg(P::IN) + i).is_zero();
    // uniform: every lane has read the same six slots, which nobody writes before the next sync
    if (zero) return false;
    // EXPX unrolls here into a copy, then per bit of BN_X from bit 61 down a cyclotomic squaring and, for a set bit, a
    // product with the base, then the conjugation (x > 0 for BN254).  pc, mode and bit are constants' children: uniform.
    int pc = 0, mode = 0, bit = 0, xo = 0, xa = 0;
    for (;;) {
        int kind, o, a, b = 0;
        if (mode == 0) {
            if (pc == P::N) break;
            kind = P::OPS[pc][0]; o = P::OPS[pc][1]; a = P::OPS[pc][2]; b = P::OPS[pc][3];
            ++pc;
            if (kind == P::EXPX) { kind = P::COPY; xo = o; xa = a; bit = 61; mode = 1; }
        } else if (mode == 1) {
            kind = P::CYC; o = a = xo;
            mode = ((PairingConsts::BN_X >> bit) & 1u) ? 2 : bit == 0 ? 3 : 1;
            if (mode == 1) --bit;
        } else if (mode == 2) {
            kind = P::MUL; o = a = xo; b = xa;
            mode = bit == 0 ? 3 : 1;
            if (mode == 1) --bit;
        } else {
            kind = P::CONJ; o = a = xo;
            mode = 0;
        }
        const int ro = tp::reg(o), ra = tp::reg(a);
        switch (kind) {
            case P::MUL: team_mul12(ln, sh, ro, ra, tp::reg(b)); break;
            case P::CYC: team_cyc_sqr(ln, sh, ro, ra); break;
            case P::CONJ: team_conj(ln, sh, ro, ra); break;
            case P::FROB: team_frob(ln, sh, ro, ra, b); break;
            case P::INV: team_inv12(ln, sh, ro, ra); break;
            default: team_phase(ln, 6, [&](int job) { sh.st(job, ro + job, sh.ld(job, ra + job)); }); break;
        }
    }
    return true;
}

// ---- the multi-Miller loop --------------------------------------------------------------------------------------------
// Pair handling as multi_miller_loop<NF>: pairs [0, NF) take their coefficients from their G2 point on the fly, the rest
// from a prepared table of 91; a pair whose `live` is false is skipped.  The result is left in slots tp::F .. tp::F + 5.
//
// A step (a doubling with f's squaring, or an addition) runs two tracks of phases side by side.  The f track: the
// coefficients of the prepared pairs scaled by their G1 points (with the 12 products of the squaring), the squaring's
// combine, then per live pair the 13 products of mul_by_034 and their combine - prepared pairs first.  The line track, on
// spare lanes, is line_double / line_add of the live on-the-fly pairs, which do not depend on f: four or five phases of at
// most seven jobs a pair.  Its coefficient, scaled, is ready after three phases; the f track waits for it only if it
// gets there sooner.
template <int NF, class L, class S>
CG_PF void team_multi_miller_loop(L& ln, S& sh, const MillerPairs& in) {
    typedef PairingConsts K;
    // the live pairs, two bits each: prepared ones first in `ord`; the live on-the-fly ones also in `fly`
    int ord = 0, nlive = 0, npre = 0, fly = 0, nfly = 0;
    for (int j = NF; j < 3; ++j)
        if (in.live[j]) { ord |= j << (2 * nlive); ++nlive; ++npre; }
    for (int j = 0; j < NF; ++j)
        if (in.live[j]) { ord |= j << (2 * nlive); ++nlive; fly |= j << (2 * nfly); ++nfly; }
    auto fly_at = [&](int w) { return tp::LN + tp::LSTRIDE * ((fly >> (2 * w)) & 3); };
    // pair j's members by selection, not by an index known only at run time: `in` then needs no private segment
    auto tab_of = [&](int j) { return j == 0 ? in.tab[0] : j == 1 ? in.tab[1] : in.tab[2]; };
    auto g1_of = [&](int j) { return Fq2{select(j == 0, in.p[0].x, select(j == 1, in.p[1].x, in.p[2].x)), select(j == 0, in.p[0].y, select(j == 1, in.p[1].y, in.p[2].y))}; };
    auto g2x_of = [&](int j) { return select(j == 0, in.q[0].x, select(j == 1, in.q[1].x, in.q[2].x)); };
    auto g2y_of = [&](int j) { return select(j == 0, in.q[0].y, select(j == 1, in.q[1].y, in.q[2].y)); };

    // f = 1, the G1 points, r = q
    team_phase(ln, 6 + 3 + nfly, [&](int job) {
        if (job < 6) { sh.st(job, tp::F + job, job == 0 ? Fq2::one() : Fq2::zero()); return; }
        if (job < 9) { sh.st(job, tp::P + job - 6, g1_of(job - 6)); return; }
        const int w = job - 9, j = (fly >> (2 * w)) & 3, at = fly_at(w);
        const Fq2 qx = g2x_of(j), qy = g2y_of(j);
        sh.st(job, at + tp::RX, qx);
        sh.st(job, at + tp::RY, qy);
        sh.st(job, at + tp::RZ, Fq2::one());
        sh.st(job, at + tp::QX, qx);
        sh.st(job, at + tp::QY, qy);
    });
    // q1 = mul_by_char(q), q2 = -mul_by_char(q1) (y negated), for the two last additions
    for (int round = 0; round < 2; ++round)
        team_phase(ln, 2 * nfly, [&](int job) {
            const int at = fly_at(job >> 1), y = job & 1;
            const Fq2 v = mul(conj(sh.ld(job, at + (round ? tp::Q1X : tp::QX) + y)), fq2_const(y ? K::TWIST_MUL_BY_Q_Y : K::FROB6_C1_1));
            sh.st(job, at + (round ? tp::Q2X : tp::Q1X) + y, round && y ? neg(v) : v);
        });

    // one line-track job: q = job within the pair's stage, at = the pair's slots, pj = its G1 point's slot
    auto line_dbl = [&](int job, int stage, int q, int at, int pj) -> TeamJob {
        auto V = [&](int s) { return sh.ld(job, at + s); };
        if (stage == 0) {
            if (q == 0) return team_product(at + tp::DA, fq2_half(V(tp::RX)), V(tp::RY));
            if (q == 4) { const Fq2 s = add(V(tp::RY), V(tp::RZ)); return team_product(at + tp::DHS, s, s); }
            const Fq2 v = V(q == 1 ? tp::RY : q == 2 ? tp::RZ : tp::RX);
            return team_product(at + (q == 1 ? tp::DB : q == 2 ? tp::DC : tp::DJ), v, v);
        }
        if (stage == 1) {
            const Fq2 c = V(tp::DC);
            return team_product(at + tp::DE, fq2_const(K::TWIST_B), add(dbl(c), c));
        }
        if (stage == 2) {
            const Fq2 b = V(tp::DB), e = V(tp::DE);
            const Fq2 f = add(dbl(e), e);
            auto H = [&]() { return sub(V(tp::DHS), add(b, V(tp::DC))); };
            if (q == 0) return team_product(at + tp::CO0, neg(H()), fq2_of(sh.ld(job, pj).c1));
            if (q == 1) { const Fq2 j = V(tp::DJ); return team_product(at + tp::CO3, add(dbl(j), j), fq2_of(sh.ld(job, pj).c0)); }
            if (q == 2) return team_value(at + tp::CO4, sub(e, b));
            if (q == 3) return team_product(at + tp::RX, V(tp::DA), sub(b, f));
            if (q == 4) { const Fq2 g = fq2_half(add(b, f)); return team_product(at + tp::DGS, g, g); }
            if (q == 5) return team_product(at + tp::DES, e, e);
            return team_product(at + tp::RZ, b, H());
        }
        const Fq2 es = V(tp::DES);
        return team_value(at + tp::RY, sub(V(tp::DGS), add(dbl(es), es)));
    };
    // qsel: 0 = +q, 1 = -q, 2 = q1, 3 = q2
    auto line_add_job = [&](int job, int stage, int q, int at, int pj, int qsel) -> TeamJob {
        auto V = [&](int s) { return sh.ld(job, at + s); };
        auto QXv = [&]() { return V(qsel < 2 ? tp::QX : qsel == 2 ? tp::Q1X : tp::Q2X); };
        auto QYv = [&]() { const Fq2 y = V(qsel < 2 ? tp::QY : qsel == 2 ? tp::Q1Y : tp::Q2Y); return qsel == 1 ? neg(y) : y; };
        auto THETA = [&]() { return sub(V(tp::RY), V(tp::AM1)); };
        auto LAMBDA = [&]() { return sub(V(tp::RX), V(tp::AM2)); };
        if (stage == 0) return team_product(at + (q == 0 ? tp::AM1 : tp::AM2), q == 0 ? QYv() : QXv(), V(tp::RZ));
        if (stage == 1) {
            if (q == 0) { const Fq2 t = THETA(); return team_product(at + tp::AC, t, t); }
            if (q == 1) { const Fq2 l = LAMBDA(); return team_product(at + tp::AD, l, l); }
            if (q == 2) return team_product(at + tp::AJ1, THETA(), QXv());
            return team_product(at + tp::AJ2, LAMBDA(), QYv());
        }
        if (stage == 2) {
            if (q == 0) return team_product(at + tp::AE, LAMBDA(), V(tp::AD));
            if (q == 1) return team_product(at + tp::AF, V(tp::RZ), V(tp::AC));
            if (q == 2) return team_product(at + tp::AG, V(tp::RX), V(tp::AD));
            if (q == 3) return team_product(at + tp::CO0, LAMBDA(), fq2_of(sh.ld(job, pj).c1));
            if (q == 4) return team_product(at + tp::CO3, neg(THETA()), fq2_of(sh.ld(job, pj).c0));
            return team_value(at + tp::CO4, sub(V(tp::AJ1), V(tp::AJ2)));
        }
        if (stage == 3) {
            const Fq2 e = V(tp::AE), g = V(tp::AG);
            auto H = [&]() { return sub(add(e, V(tp::AF)), dbl(g)); };
            if (q == 0) return team_product(at + tp::ANX, LAMBDA(), H());
            if (q == 1) return team_product(at + tp::AT1, THETA(), sub(g, H()));
            if (q == 2) return team_product(at + tp::AT2, e, V(tp::RY));
            return team_product(at + tp::ANZ, V(tp::RZ), e);
        }
        if (q == 0) return team_value(at + tp::RX, V(tp::ANX));
        if (q == 1) return team_value(at + tp::RY, sub(V(tp::AT1), V(tp::AT2)));
        return team_value(at + tp::RZ, V(tp::ANZ));
    };

    // one step over coefficient k: a doubling (with f's squaring) or an addition of the addend `qsel`
    auto step = [&](bool dbl_step, int qsel, int k) {
        const int n_line = nfly ? (dbl_step ? 4 : 5) : 0;
        const int head = dbl_step ? 2 : (npre ? 1 : 0);
        const int n_f = head + 2 * nlive;
        int fs = 0, ls = 0;
        // uniform: the bounds and every condition below come from the live flags and the step's kind alone
        while (fs < n_f || ls < n_line) {
            bool run_f = fs < n_f;
            int pair = 0, fjobs = 0;
            bool comb = false;
            if (run_f && fs >= head) {
                pair = (ord >> (2 * ((fs - head) >> 1))) & 3;
                comb = (fs - head) & 1;
                if (!comb && pair < NF && ls < 3) run_f = false;        // the line track has not scaled its coefficient yet
                fjobs = comb ? 6 : 13;
            } else if (run_f) {
                fjobs = fs == 0 ? (dbl_step ? 12 : 0) + 2 * npre : 6;
            }
            if (!run_f) fjobs = 0;
            const int per_pair = dbl_step ? (ls == 0 ? 5 : ls == 1 ? 1 : ls == 2 ? 7 : 1) : (ls == 0 ? 2 : ls == 1 ? 4 : ls == 2 ? 6 : ls == 3 ? 4 : 3);
            const int ljobs = ls < n_line ? nfly * per_pair : 0;
            for (int job = ln.lane; job < fjobs + ljobs; job += ln.nl) {
                TeamJob jb;
                if (job >= fjobs) {
                    const int e = job - fjobs, w = e / per_pair, q = e % per_pair;
                    const int at = fly_at(w), pj = tp::P + ((fly >> (2 * w)) & 3);
                    jb = dbl_step ? line_dbl(job, ls, q, at, pj) : line_add_job(job, ls, q, at, pj, qsel);
                } else if (fs < head) {
                    if (fs == 1) {
                        jb = sqr12_comb(sh, job, job, tp::F);
                    } else if (dbl_step && job < 12) {
                        jb = sqr12_prod(sh, job, job, tp::F);
                    } else {                                            // c0·y_P or c1·x_P of a prepared pair's coefficient
                        const int e = job - (dbl_step ? 12 : 0), j = (ord >> (2 * (e >> 1))) & 3;
                        const Fq2 pt = sh.ld(job, tp::P + j);
                        const EllCoeff* c = tab_of(j) + k;
                        jb = team_product(tp::D + 2 * j + (e & 1), (e & 1) ? c->c1 : c->c0, fq2_of((e & 1) ? pt.c0 : pt.c1));
                    }
                } else if (comb) {
                    jb = ell_comb(sh, job, job);
                } else {
                    Fq2 d0, d3, d4;
                    if (pair < NF) {
                        const int at = tp::LN + tp::LSTRIDE * pair;
                        d0 = sh.ld(job, at + tp::CO0); d3 = sh.ld(job, at + tp::CO3); d4 = sh.ld(job, at + tp::CO4);
                    } else {
                        d0 = sh.ld(job, tp::D + 2 * pair); d3 = sh.ld(job, tp::D + 2 * pair + 1); d4 = tab_of(pair)[k].c2;
                    }
                    jb = ell_prod(sh, job, job, d0, d3, d4);
                }
                team_finish(sh, job, jb);                               // the phase's one product
            }
            ln.sync();
            if (run_f) ++fs;
            if (ls < n_line) ++ls;
        }
    };

    // the 91 coefficients in consumption order: a doubling per digit (the first squaring is of f = 1), an addition after a
    // non-zero digit, the two last additions.  One call of `step` in the source: the kernel holds its code once.
    int i = K::ATE_TOP, d = 0;
    for (int k = 0; k < K::N_COEFFS; ++k) {
        bool dbl_step = false;
        int qsel = 0;
        if (k >= K::N_COEFFS - 2) {
            qsel = k - (K::N_COEFFS - 4);
        } else if (d != 0) {
            qsel = d > 0 ? 0 : 1;
            d = 0;
        } else {
            d = ate_digit(--i);
            dbl_step = true;
        }
        step(dbl_step, qsel, k);
    }
}

#if defined(__HIPCC__)
// ---- the device's team: ONE workgroup of one wave per proof; values cross lanes through LDS only ----------------------
constexpr int TEAM_WIDTH = 64;
struct WaveLane {
    int lane;
    static constexpr int nl = TEAM_WIDTH;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};
// The bodies of the verifiers' team kernels (verify.hip, rangeverify.hip), entered by the whole workgroup together: the
// callers' early returns come before them and are uniform.
template <int NF>
__device__ __forceinline__ void team_miller_to(TeamMem& sh, const MillerPairs& mp, Fq12* out) {
    WaveLane ln{(int)threadIdx.x};
    team_multi_miller_loop<NF>(ln, sh, mp);               // ends with a sync
    if (ln.lane < 6) reinterpret_cast<Fq2*>(out)[ln.lane] = sh.v[tp::F + ln.lane];
}
// final exponentiation of *f; `some` = false for f = 0, else the value is in register 0.  Every lane returns the same.
__device__ __forceinline__ bool team_final_of(TeamMem& sh, WaveLane& ln, const Fq12* f) {
    if (ln.lane < 6) sh.v[tp::reg(9) + ln.lane] = reinterpret_cast<const Fq2*>(f)[ln.lane];
    ln.sync();
    return team_final_exponentiation(ln, sh);
}
#endif

}  // namespace cg
