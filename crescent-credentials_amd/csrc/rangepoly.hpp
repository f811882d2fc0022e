// The polynomial stage of `RangeProof::prove_n_bits` (creds/src/rangeproof.rs:141-325) over Fr: from one Pedersen opening,
// its 18 random scalars and the two challenges to the scalar of every fixed-base term of the proof's points
// (csrc/rangeproof.hip walks the tables), the three evaluations and the three random_v.
//
//   g~ = ifft(suffix sums of m's bits) + (b0 + b1 X + b2 X^2)(X^n - 1)                     n + 3 coefficients
//   q1 = (g~ - m)/(X - 1)        q2 = g~(1 - g~)/(X - w^(n-1))
//   q3 = h(1 - h)(X - w^(n-1))/(X^n - 1),  h = g~(X) - 2 g~(wX)
//   q  = q1 + c q2 + c^2 q3                                                                2n + 4 coefficients
//   w^ = f_coeff m + q_coeff q,  q_coeff = rho^n - 1,  f_coeff = q_coeff/(rho - 1)
//   open(p, z, rand): p/(X - z), rand/(X - z), p(z), rand(z)   (forks/ark-poly-commit/src/kzg10/mod.rs:247-331)
// All three divisions are exact for m < 2^n; only quotients are used, as in the reference.  Vectors keep their full
// length: a zero blinding leaves zero top coefficients, which the group stage skips.
//
// The code is written once for "lanes": every loop over output coefficients is strided by L::nl from L::lane, and
// L::sync() separates a step from the one that reads it.  On the device a lane is a lane of the one wave that owns a
// showing and the vectors live in LDS; on the host there is one lane (HostLane) and the same code is a plain loop, which
// is how tests/cpp/test_rangepoly.cpp runs it under g++.  The inverse transform is the direct O(n^2) sum (n <= 32), the
// products are schoolbook, a division by a linear factor is Horner's rule (one lane each; independent divisions run on
// neighbouring lanes), the division by X^n - 1 a fold per residue class.
#pragma once
#include "field.hpp"

namespace cg {

constexpr int RP_MAX_BITS = 32;                       // RANGE_PROOF_INTERVAL_BITS; the reference needs a power of two below 64
constexpr int RP_G_LEN = RP_MAX_BITS + 3;             // g~, h
constexpr int RP_Q_LEN = 2 * RP_MAX_BITS + 4;         // q, w^
constexpr int RP_P_LEN = 2 * RP_MAX_BITS + 6;         // the longest product: h(1 - h)(X - w^(n-1))
constexpr int RP_N_RAND = 18, RP_N_RESP = 6;
// the rand row, in the order the reference draws it
enum { RP_B = 0, RP_F = 3, RP_TM = 6, RP_TR = 7, RP_TF = 8, RP_G = 11, RP_Q = 15 };

// terms per showing of each call, and where a point's terms start (the group stage's descriptor follows these)
CG_HD constexpr uint32_t rp_commit_terms(uint32_t n) { return n + 17; }      // com_f 4 | com_g n + 7 | k_0 2 | k_1 4
CG_HD constexpr uint32_t rp_quotient_terms(uint32_t n) { return 2 * n + 7; } // com_q: q, then rand_q
CG_HD constexpr uint32_t rp_open_terms(uint32_t n) { return 4 * n + 15; }    // W_g n + 5 | W_gw n + 5 | W_w^ 2n + 5

struct RangeConsts {          // of one domain size, Montgomery form
    uint32_t n, log_n;
    Fr w, w_inv, n_inv;       // the domain's generator, w^-1 = w^(n-1), 1/n
};

struct RangeWork {            // one showing's vectors, Montgomery form: 9 KB
    Fr g[RP_G_LEN];           // g~
    Fr h[RP_G_LEN];           // the suffix sums, then g~(X) - 2 g~(wX)
    Fr p[RP_P_LEN];           // a product, then q3
    Fr t[RP_P_LEN];           // q2, then h(1 - h)(X - w^(n-1))
    Fr q[RP_Q_LEN];           // q1, q, then w^
    Fr r[7];                  // rand_g (4), then rand_w^ (3)
};

struct RangeIn {              // canonical scalars as the caller passed them, 8 words each
    const uint32_t* open;     // m, r
    const uint32_t* rand;     // RP_N_RAND
    const uint32_t* c;        // unused by the commit call
    const uint32_t* rho;      // used by the open call only
};

struct HostLane {
    static constexpr int lane = 0, nl = 1;
    void sync() const {}
};

CG_HD Fr rp_load(const uint32_t* w) {
    Fr a;
#pragma unroll
    for (int i = 0; i < 8; ++i) a.l[i] = w[i];
    return a;
}
CG_HD void rp_store(uint32_t* w, const Fr& a) {
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = a.l[i];
}
CG_HD bool rp_below_r(const uint32_t* a) {
    for (int i = 7; i >= 0; --i) {
        if (a[i] < FrP::N[i]) return true;
        if (a[i] > FrP::N[i]) return false;
    }
    return false;
}
CG_HD bool rp_all_zero(const uint32_t* a, int count) {
    uint32_t o = 0;
    for (int i = 0; i < 8 * count; ++i) o |= a[i];
    return o == 0;
}
CG_HD Fr rp_pow(const Fr& a, uint32_t e) {
    Fr r = Fr::one(), s = a;
    for (; e; e >>= 1) {
        if (e & 1u) r = mul(r, s);
        s = sqr(s);
    }
    return r;
}

// what makes a showing CG_SHOW_MALFORMED before any arithmetic: a scalar >= r, m >= 2^n, or a blinding polynomial that is
// zero (the reference would emit a non-hiding commitment and random_v = None).  c and rho are looked at when given.
CG_HD bool rp_inputs_ok(uint32_t n, const RangeIn& in) {
    bool ok = rp_below_r(in.open) && rp_below_r(in.open + 8);
    for (int j = 0; j < RP_N_RAND; ++j) ok = ok && rp_below_r(in.rand + 8 * j);
    if (in.c) ok = ok && rp_below_r(in.c);
    if (in.rho) ok = ok && rp_below_r(in.rho);
    uint32_t high = n >= 32 ? 0u : in.open[0] >> n;            // m < 2^n (groth16rand.rs:202-204)
    for (int i = 1; i < 8; ++i) high |= in.open[i];
    ok = ok && high == 0;
    ok = ok && !rp_all_zero(in.rand + 8 * RP_F, 3) && !rp_all_zero(in.rand + 8 * RP_G, 4) && !rp_all_zero(in.rand + 8 * RP_Q, 3);
    return ok;
}

// the constants of the size-n domain, n = 2^log_n <= 32: w = 5^((r - 1)/n) as ark-ff derives it (Fr::GENERATOR = 5)
inline RangeConsts range_consts(uint32_t log_n) {
    RangeConsts k;
    k.n = 1u << log_n;
    k.log_n = log_n;
    uint32_t e[8];
    for (int i = 0; i < 8; ++i) e[i] = FrP::N[i];
    e[0] -= 1u;
    for (int i = 0; i < 8; ++i) e[i] = (e[i] >> log_n) | (i < 7 && log_n ? e[i + 1] << (32 - log_n) : 0u);
    Fr five = Fr::zero(), nn = Fr::zero();
    five.l[0] = 5;
    nn.l[0] = k.n;
    k.w = pow_limbs(to_mont(five), e);
    k.w_inv = inv(k.w);
    k.n_inv = inv(to_mont(nn));
    return k;
}

// src/(X - z) for len coefficients: the quotient's len - 1 coefficients to qm (Montgomery) and / or qc (canonical words),
// the remainder src(z) to rem (canonical words)
CG_HD void rp_div_linear(const Fr* src, int len, const Fr& z, Fr* qm, uint32_t* qc, uint32_t* rem) {
    Fr carry = Fr::zero();
    for (int i = len - 1; i >= 1; --i) {
        carry = add(src[i], mul(z, carry));
        if (qm) qm[i - 1] = carry;
        if (qc) rp_store(qc + 8 * (i - 1), from_mont(carry));
    }
    if (rem) rp_store(rem, from_mont(add(src[0], mul(z, carry))));
}

// p = a(1 - a): 2 len - 1 coefficients, one per lane
template <class L>
CG_HD void rp_x_one_minus_x(const Fr* a, int len, Fr* p, L& ln) {
    for (int o = ln.lane; o < 2 * len - 1; o += ln.nl) {
        const int lo = o < len ? 0 : o - len + 1, hi = o < len ? o : len - 1;
        Fr acc = Fr::zero();
        for (int i = lo; i <= hi; ++i) acc = add(acc, mul(a[i], a[o - i]));
        p[o] = sub(o < len ? a[o] : Fr::zero(), acc);
    }
}

// W.g = g~ (rangeproof.rs:143-172).  m < 2^n <= 2^32: the suffix sum from bit i is m >> i.
template <class L>
CG_HD void rp_g_blinded(const RangeConsts& k, const RangeIn& in, RangeWork& W, L& ln) {
    const int n = (int)k.n;
    const uint32_t m = in.open[0];
    for (int i = ln.lane; i < n; i += ln.nl) {
        Fr e = Fr::zero();
        e.l[0] = m >> i;
        W.h[i] = to_mont(e);
    }
    ln.sync();
    for (int j = ln.lane; j < n + 3; j += ln.nl) {
        Fr acc = Fr::zero();
        if (j < n) {
            const Fr step = rp_pow(k.w_inv, (uint32_t)j);
            for (int i = n - 1; i >= 0; --i) acc = add(mul(acc, step), W.h[i]);
            acc = mul(acc, k.n_inv);
        }
        W.g[j] = acc;
    }
    ln.sync();
    if (ln.lane == 0) {            // in turn: at n = 2 the two halves of the blinding overlap
        for (int i = 0; i < 3; ++i) {
            const Fr b = to_mont(rp_load(in.rand + 8 * (RP_B + i)));
            W.g[i] = sub(W.g[i], b);
            W.g[n + i] = add(W.g[n + i], b);
        }
    }
    ln.sync();
}

// W.q = q (rangeproof.rs:183-266), after rp_g_blinded
template <class L>
CG_HD void rp_quotient(const RangeConsts& k, const RangeIn& in, RangeWork& W, L& ln) {
    const int n = (int)k.n;
    const Fr c = to_mont(rp_load(in.c));
    for (int i = ln.lane; i < n + 3; i += ln.nl) W.h[i] = sub(W.g[i], dbl(mul(W.g[i], rp_pow(k.w, (uint32_t)i))));
    for (int i = n + 2 + ln.lane; i < 2 * n + 4; i += ln.nl) W.q[i] = Fr::zero();
    rp_x_one_minus_x(W.g, n + 3, W.p, ln);
    ln.sync();
    // q1 = (g~ - m)/(X - 1) (the constant term only reaches the remainder) and q2 = g~(1 - g~)/(X - w^(n-1))
    for (int job = ln.lane; job < 2; job += ln.nl)
        rp_div_linear(job ? W.p : W.g, job ? 2 * n + 5 : n + 3, job ? k.w_inv : Fr::one(), job ? W.t : W.q, nullptr, nullptr);
    ln.sync();
    for (int i = ln.lane; i < 2 * n + 4; i += ln.nl) W.q[i] = add(W.q[i], mul(c, W.t[i]));
    rp_x_one_minus_x(W.h, n + 3, W.p, ln);
    ln.sync();
    for (int o = ln.lane; o < 2 * n + 6; o += ln.nl)          // times (X - w^(n-1))
        W.t[o] = sub(o > 0 ? W.p[o - 1] : Fr::zero(), o < 2 * n + 5 ? mul(k.w_inv, W.p[o]) : Fr::zero());
    ln.sync();
    for (int r = ln.lane; r < n; r += ln.nl)                  // by X^n - 1: q3[i] = t[i + n] + q3[i + n], n + 6 coefficients
        for (int i = r + (n + 5 - r) / n * n; i >= 0; i -= n) W.p[i] = add(W.t[i + n], i + n < n + 6 ? W.p[i + n] : Fr::zero());
    ln.sync();
    const Fr c2 = sqr(c);
    for (int i = ln.lane; i < n + 6; i += ln.nl) W.q[i] = add(W.q[i], mul(c2, W.p[i]));
    ln.sync();
}

// ---- the three calls: false = CG_SHOW_MALFORMED, and nothing is written then --------------------------------------------
// terms: rp_commit_terms(n) x 8 canonical words: m f0 f1 f2 | g~, g0..g3 | t_m t_r | t_f0 t_f1 t_f2 t_m
template <class L>
CG_HD bool rp_commit(const RangeConsts& k, const RangeIn& in0, RangeWork& W, uint32_t* terms, L& ln) {
    const RangeIn in{in0.open, in0.rand, nullptr, nullptr};
    if (!rp_inputs_ok(k.n, in)) return false;
    const int n = (int)k.n;
    rp_g_blinded(k, in, W, ln);
    for (int i = ln.lane; i < n + 3; i += ln.nl) rp_store(terms + 8 * (4 + i), from_mont(W.g[i]));
    for (int t = ln.lane; t < 14; t += ln.nl) {             // the terms that are inputs as they came
        static constexpr int8_t SRC[14] = {-1, RP_F, RP_F + 1, RP_F + 2, RP_G, RP_G + 1, RP_G + 2, RP_G + 3,
                                           RP_TM, RP_TR, RP_TF, RP_TF + 1, RP_TF + 2, RP_TM};
        const int at = t < 4 ? t : t + n + 3;
        const uint32_t* s = SRC[t] < 0 ? in.open : in.rand + 8 * SRC[t];
        for (int l = 0; l < 8; ++l) terms[8 * at + l] = s[l];
    }
    return true;
}

// terms: rp_quotient_terms(n) x 8: q, then q0 q1 q2
template <class L>
CG_HD bool rp_quotient_call(const RangeConsts& k, const RangeIn& in0, RangeWork& W, uint32_t* terms, L& ln) {
    const RangeIn in{in0.open, in0.rand, in0.c, nullptr};
    if (!rp_inputs_ok(k.n, in)) return false;
    const int n = (int)k.n;
    rp_g_blinded(k, in, W, ln);
    rp_quotient(k, in, W, ln);
    for (int i = ln.lane; i < 2 * n + 4; i += ln.nl) rp_store(terms + 8 * i, from_mont(W.q[i]));
    for (int t = ln.lane; t < 24; t += ln.nl) terms[8 * (2 * n + 4) + t] = in.rand[8 * RP_Q + t];
    return true;
}

// terms: rp_open_terms(n) x 8: g~/(X - rho), rand_g/(X - rho) | the same at rho w | w^/(X - rho), rand_w^/(X - rho)
// evals: 3 x 8 words (eval_g, eval_gw, eval_w^); proofs: 3 x 24 words, random_v in words 16..23 of each
template <class L>
CG_HD bool rp_open(const RangeConsts& k, const RangeIn& in, RangeWork& W, uint32_t* terms, uint32_t* evals, uint32_t* proofs, L& ln) {
    if (!rp_inputs_ok(k.n, in)) return false;
    const int n = (int)k.n;
    const Fr rho = to_mont(rp_load(in.rho));
    Fr rho_n = rho;
    for (uint32_t i = 0; i < k.log_n; ++i) rho_n = sqr(rho_n);
    if (rho_n == Fr::one()) return false;                    // rho = 1 among them: the reference divides by rho - 1
    rp_g_blinded(k, in, W, ln);
    rp_quotient(k, in, W, ln);
    const Fr q_coeff = sub(rho_n, Fr::one());
    const Fr f_coeff = mul(q_coeff, inv(sub(rho, Fr::one())));
    for (int i = ln.lane; i < 2 * n + 4; i += ln.nl) {
        Fr v = mul(q_coeff, W.q[i]);
        if (i == 0) v = add(v, mul(f_coeff, to_mont(rp_load(in.open))));
        W.q[i] = v;
    }
    for (int j = ln.lane; j < 7; j += ln.nl)
        W.r[j] = j < 4 ? to_mont(rp_load(in.rand + 8 * (RP_G + j)))
                       : add(mul(f_coeff, to_mont(rp_load(in.rand + 8 * (RP_F + j - 4)))), mul(q_coeff, to_mont(rp_load(in.rand + 8 * (RP_Q + j - 4)))));
    ln.sync();
    const Fr rho_w = mul(rho, k.w);
    for (int job = ln.lane; job < 6; job += ln.nl) {
        const int pt = job % 3;                              // proof_g, proof_gw, proof_w^
        const bool blind = job >= 3;
        const int at = pt == 0 ? 0 : pt == 1 ? n + 5 : 2 * n + 10;             // the point's first term
        const int wit_len = pt == 2 ? 2 * n + 4 : n + 3;
        const Fr* src = blind ? (pt == 2 ? W.r + 4 : W.r) : (pt == 2 ? W.q : W.g);
        rp_div_linear(src, blind ? (pt == 2 ? 3 : 4) : wit_len, pt == 1 ? rho_w : rho, nullptr,
                      terms + 8 * (at + (blind ? wit_len - 1 : 0)), blind ? proofs + 24 * pt + 16 : evals + 8 * pt);
    }
    return true;
}

}  // namespace cg
