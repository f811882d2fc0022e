// The group of P-256 (secp256r1), y^2 = x^3 - 3x + b over fp256.hpp's field, of prime order n (fq256.hpp), written once for
// host and device; and on it the two host steps in front of pi2: `compute_TU` and `compute_RTU`
// (ecdsa-pop/src/lib.rs:217-240 and :180-215), cut into the pieces csrc/p256tu.hip runs as kernels and put together again
// as whole rows for the host (tests/cpp/test_p256.cpp, and the single-thread figure of profiles/p256_tu.md).
//
// Coordinates: homogeneous projective (X : Y : Z), the identity (0 : 1 : 0), with the COMPLETE addition of Renes, Costello
// and Batina (Eurocrypt 2016, section 3) specialised to a = -3.  With
//     xx = X1 X2, yy = Y1 Y2, zz = Z1 Z2, xy = X1 Y2 + X2 Y1, xz = X1 Z2 + X2 Z1, yz = Y1 Z2 + Y2 Z1,
//     A = 3 (b zz - xz), B = 3 (b xz - xx - 3 zz), C = 3 (xx - zz)
// the sum is X3 = xy (yy - A) - yz B, Y3 = (yy + A)(yy - A) + C B, Z3 = yz (yy + A) + xy C: twelve products and two by b.
// The group has odd order, so the formula has no exceptional pair: P + P, P + (-P), P + O, O + P and O + O all go through the
// same straight line, which is why it was chosen over a branched Jacobian addition - in `compute_RTU` the sum u G + v Q meets
// those cases whenever Q is a small multiple of +-G, and a signer chooses Q.  The price is the doubling: fourteen products
// through the same formula where Jacobian coordinates take eight.  A doubling IS the addition here, P + P, so that a chain is
// one addition site in a rolled loop: an addition is some 50 KB of code with every product inlined.  There is no point (x, 0) on
// this curve (odd order: no point of order two), so Y = 0 never meets the doubling.
// The mixed addition takes an affine second operand (Z2 = 1: eleven products and two by b); an affine point cannot be the
// identity, and a fixed-base walk skips the windows whose digit is zero.
//
// Fixed base G: 8-bit windows, 32 rows of 255 affine points, row w entry d - 1 being d·2^(8w)·G, built on the host once per
// process from G's two coordinates alone, by additions and ONE batched inversion (fixed_base.hpp's host build does the same
// for BN254), 522 240 bytes.  Variable base: a fixed 4-bit window over 256 bits; the sixteen multiples of the base are a
// per-lane table in memory the caller provides, ENTRY-MAJOR (entry e of lane p at e·stride + p) - sixteen projective points
// are 384 words, which registers do not hold and scratch must not.  Every lane runs the same 14 + 320 additions.
// Constant time is not a requirement: every input is public.
//
// Scalars and digits are read through pointers to canonical words in memory, never out of a per-lane array indexed by a
// run-time value: the kernels that inline this declare no private segment.
#pragma once
#include <vector>

#include "fp256.hpp"
#include "fq256.hpp"

namespace cg {

struct P256Affine {
    F256 x, y;                             // Montgomery form; never the identity
};
struct P256Point {
    F256 x, y, z;                          // (X : Y : Z), Montgomery form; the identity is (0 : 1 : 0)
};
// what the formulas need of the curve, in Montgomery form: b and 1.  Two products per lane, once.
struct P256Curve {
    F256 b, one;
};

constexpr int P256_WINDOWS = 32, P256_ROW = 255;
constexpr int P256_TABLE_POINTS = P256_WINDOWS * P256_ROW;
constexpr int P256_CHAIN_TABLE = 16;       // entries of a variable-base chain's table
enum : uint8_t { P256_MADE = 1, P256_MALFORMED = 2, P256_BAD_SIGNATURE = 3 };      // the status bytes of include/crescent_gpu.h

CG_HD constexpr uint32_t p256_b(int i) {
    constexpr uint32_t b[8] = {0x27d2604bu, 0x3bce3c3eu, 0xcc53b0f6u, 0x651d06b0u, 0x769886bcu, 0xb3ebbd55u, 0xaa3a93e7u, 0x5ac635d8u};
    return b[i];
}
CG_HD constexpr uint32_t p256_gx(int i) {
    constexpr uint32_t x[8] = {0xd898c296u, 0xf4a13945u, 0x2deb33a0u, 0x77037d81u, 0x63a440f2u, 0xf8bce6e5u, 0xe12c4247u, 0x6b17d1f2u};
    return x[i];
}
CG_HD constexpr uint32_t p256_gy(int i) {
    constexpr uint32_t y[8] = {0x37bf51f5u, 0xcbb64068u, 0x6b315eceu, 0x2bce3357u, 0x7c0f9e16u, 0x8ee7eb4au, 0xfe1a7f9bu, 0x4fe342e2u};
    return y[i];
}

CG_HD P256Curve p256_curve() {
    P256Curve c;
    F256 b, one = f256_zero();
#pragma unroll
    for (int i = 0; i < 8; ++i) b.l[i] = p256_b(i);
    one.l[0] = 1;
    c.b = f256_to_mont(b);
    c.one = f256_to_mont(one);
    return c;
}
CG_HD bool f256_is_zero(const F256& a) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) o |= a.l[i];
    return o == 0;
}
CG_HD P256Point p256_identity(const P256Curve& c) { return P256Point{f256_zero(), c.one, f256_zero()}; }
CG_HD bool p256_is_identity(const P256Point& p) { return f256_is_zero(p.z); }
CG_HD P256Point p256_from_affine(const P256Affine& a, const P256Curve& c) { return P256Point{a.x, a.y, c.one}; }
CG_HD P256Affine p256_neg(const P256Affine& a) { return P256Affine{a.x, f256_neg(a.y)}; }
CG_HD P256Affine p256_generator() {
    F256 x, y;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        x.l[i] = p256_gx(i);
        y.l[i] = p256_gy(i);
    }
    return P256Affine{f256_to_mont(x), f256_to_mont(y)};
}
// y^2 = x^3 - 3x + b
CG_HD bool p256_on_curve(const P256Affine& a, const P256Curve& c) {
    const F256 x2 = f256_sqr(a.x);
    F256 rhs = f256_mul(x2, a.x);
    const F256 x3 = f256_add(f256_add(a.x, a.x), a.x);
    rhs = f256_add(f256_sub(rhs, x3), c.b);
    return f256_eq(f256_sqr(a.y), rhs);
}

CG_HD F256 f256_triple(const F256& a) { return f256_add(f256_add(a, a), a); }
// the second half of both additions: the header has the formula
CG_HD P256Point p256_add_tail(const F256& xx, const F256& yy, const F256& zz, const F256& xy, const F256& xz, const F256& yz, const P256Curve& c) {
    const F256 A = f256_triple(f256_sub(f256_mul(c.b, zz), xz));
    const F256 B = f256_triple(f256_sub(f256_sub(f256_mul(c.b, xz), xx), f256_triple(zz)));
    const F256 C = f256_triple(f256_sub(xx, zz));
    const F256 lo = f256_sub(yy, A), up = f256_add(yy, A);
    P256Point r;
    r.x = f256_sub(f256_mul(xy, lo), f256_mul(yz, B));
    r.y = f256_add(f256_mul(up, lo), f256_mul(C, B));
    r.z = f256_add(f256_mul(yz, up), f256_mul(xy, C));
    return r;
}
// the general, complete addition: any two points of the group, equal, opposite or the identity
CG_HD P256Point p256_add(const P256Point& p, const P256Point& q, const P256Curve& c) {
    const F256 xx = f256_mul(p.x, q.x), yy = f256_mul(p.y, q.y), zz = f256_mul(p.z, q.z);
    const F256 xy = f256_sub(f256_sub(f256_mul(f256_add(p.x, p.y), f256_add(q.x, q.y)), xx), yy);
    const F256 xz = f256_sub(f256_sub(f256_mul(f256_add(p.x, p.z), f256_add(q.x, q.z)), xx), zz);
    const F256 yz = f256_sub(f256_sub(f256_mul(f256_add(p.y, p.z), f256_add(q.y, q.z)), yy), zz);
    return p256_add_tail(xx, yy, zz, xy, xz, yz, c);
}
CG_HD P256Point p256_double(const P256Point& p, const P256Curve& c) { return p256_add(p, p, c); }
// the same against an affine point (Z2 = 1), complete for every p, the identity included
CG_HD P256Point p256_add_mixed(const P256Point& p, const P256Affine& q, const P256Curve& c) {
    const F256 xx = f256_mul(p.x, q.x), yy = f256_mul(p.y, q.y);
    const F256 xy = f256_sub(f256_sub(f256_mul(f256_add(p.x, p.y), f256_add(q.x, q.y)), xx), yy);
    const F256 xz = f256_add(p.x, f256_mul(q.x, p.z));
    const F256 yz = f256_add(p.y, f256_mul(q.y, p.z));
    return p256_add_tail(xx, yy, p.z, xy, xz, yz, c);
}

// (X : Y : Z) with Z^-1 given -> the canonical words of x and y; the identity (Z = 0, and any zinv) -> zeros, which is what
// halo2curves' `to_affine` returns for it (forks/halo2curves/src/derive/curve.rs:507-516)
CG_HD void p256_affine_words(const P256Point& p, const F256& zinv, uint32_t x[8], uint32_t y[8]) {
    const bool inf = p256_is_identity(p);
    f256_to_words(f256_mul(p.x, zinv), x);
    f256_to_words(f256_mul(p.y, zinv), y);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        x[i] = inf ? 0u : x[i];
        y[i] = inf ? 0u : y[i];
    }
}
// normalisation with one inversion; false for the identity, whose words are zero
CG_HD bool p256_to_affine(const P256Point& p, uint32_t x[8], uint32_t y[8]) {
    p256_affine_words(p, f256_inv_hd(p.z), x, y);
    return !p256_is_identity(p);
}

// ---- bytes --------------------------------------------------------------------------------------------------------------------
// Every P-256 quantity on the wire is 32 bytes BIG-endian (h_Q's convention, SEC1's, the 64-byte signature's)
CG_HD void p256_load_be(const uint8_t* b, uint32_t w[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
        w[i] = (uint32_t)b[31 - 4 * i] | ((uint32_t)b[30 - 4 * i] << 8) | ((uint32_t)b[29 - 4 * i] << 16) | ((uint32_t)b[28 - 4 * i] << 24);
}
CG_HD void p256_store_be(const uint32_t w[8], uint8_t* b) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        b[31 - 4 * i] = (uint8_t)w[i];
        b[30 - 4 * i] = (uint8_t)(w[i] >> 8);
        b[29 - 4 * i] = (uint8_t)(w[i] >> 16);
        b[28 - 4 * i] = (uint8_t)(w[i] >> 24);
    }
}
CG_HD void p256_zero_bytes(uint8_t* b, int n) {
    for (int i = 0; i < n; ++i) b[i] = 0;
}
// x ‖ y, 64 bytes -> the point; false if a coordinate is >= p (the reference reduces it silently; this project fails closed
// on non-canonical input, as it does for scalars >= r) or the point is not on the curve (the reference panics)
CG_HD bool p256_read_point(const uint8_t* xy, const P256Curve& c, P256Affine& out) {
    uint32_t x[8], y[8];
    p256_load_be(xy, x);
    p256_load_be(xy + 32, y);
    const bool canonical = f256_below_p(x) && f256_below_p(y);
#pragma unroll
    for (int i = 0; i < 8; ++i) {              // a non-canonical row goes on as (0, 0), which is off the curve
        x[i] = canonical ? x[i] : 0u;
        y[i] = canonical ? y[i] : 0u;
    }
    out.x = f256_from_words(x);
    out.y = f256_from_words(y);
    return canonical && p256_on_curve(out, c);
}

// ---- scalar products ------------------------------------------------------------------------------------------------------------
// k·G through the table: k is eight canonical words IN MEMORY (below n, or any 256-bit integer: the table covers them all)
CG_HD P256Point p256_walk(const P256Affine* __restrict__ tab, const uint32_t* k, const P256Curve& c) {
    P256Point acc = p256_identity(c);
#pragma unroll 1
    for (int w = 0; w < P256_WINDOWS; ++w) {
        const uint32_t d = (k[w >> 2] >> (8 * (w & 3))) & 255u;
        if (d) acc = p256_add_mixed(acc, tab[w * P256_ROW + (int)d - 1], c);
    }
    return acc;
}
// k·q by a fixed 4-bit window from the top: `tab` is room for P256_CHAIN_TABLE points, entry e at tab[e·stride].  One addition
// site: steps 0..13 fill the table (e q = (e - 1) q + q), then 64 times four doublings and the addition of the digit's entry,
// entry 0 being the identity, which the complete addition takes like any other point.
CG_HD P256Point p256_chain(const P256Affine& q, const uint32_t* k, P256Point* tab, uint64_t stride, const P256Curve& c) {
    P256Point acc = p256_from_affine(q, c);
    tab[0] = p256_identity(c);
    tab[stride] = acc;
#pragma unroll 1
    for (int s = 0; s < 14 + 320; ++s) {
        P256Point other;
        if (s < 14) {
            other = tab[stride];
        } else if ((s - 14) % 5 == 4) {
            const int w = 63 - (s - 14) / 5;
            other = tab[(uint64_t)((k[w >> 3] >> (4 * (w & 7))) & 15u) * stride];
        } else {
            other = acc;
        }
        if (s == 14) acc = other = p256_identity(c);
        acc = p256_add(acc, other, c);
        if (s < 14) tab[(uint64_t)(s + 2) * stride] = acc;
    }
    return acc;
}

// ---- compute_TU and compute_RTU, in the three stages of csrc/p256tu.hip -----------------------------------------------------------
// the scalars of a row's terms, canonical words, scalar j of a row at k + 8·j·stride
constexpr int P256_TU_CHAINS = 1, P256_TU_TERMS = 2;       // r^-1 · R; (-d r^-1) · G
constexpr int P256_RTU_CHAINS = 2, P256_RTU_TERMS = 5;     // (r/s) · Q, (1/s) · Q; (d/s) · G, (d/(r s)) · G, (-d/r) · G

// compute_TU's checks and scalars: R on the curve with canonical coordinates, r = R.x mod n not zero (the reference asserts).
// The digest is read as the reference's `from_str_vartime` reads it: an integer below 2^256 < 2n, reduced once.
CG_HD bool p256_tu_scalars(const uint8_t* r_xy, const uint8_t* digest, const P256Curve& c, P256Affine& R, uint32_t* k, uint64_t stride) {
    uint32_t w[8];
    bool ok = p256_read_point(r_xy, c, R);
    p256_load_be(r_xy, w);
    const Q256 r = q256_from_words_reduced(w);
    p256_load_be(digest, w);
    const Q256 d = q256_from_words_reduced(w);
    ok = ok && !q256_is_zero(r);
    const Q256 r_inv = q256_inv(r);
    q256_to_words(r_inv, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = w[i];
    q256_to_words(q256_neg(q256_mul(d, r_inv)), w);
#pragma unroll
    for (int i = 0; i < 8; ++i) k[8 * stride + i] = w[i];
    return ok;
}
// compute_RTU's: Q as R above, r and s in [1, n - 1]; one inversion, of r·s, serves both.  T = r^-1 · R is taken apart as
// (d / (r s)) · G + (1 / s) · Q, so that it waits for no other term.  r_words: r as canonical words, for the last comparison.
CG_HD bool p256_rtu_scalars(const uint8_t* q_xy, const uint8_t* sig, const uint8_t* digest, const P256Curve& c, P256Affine& Q, uint32_t* k,
                            uint64_t stride, uint32_t* r_words) {
    uint32_t w[8], ws[8];
    bool ok = p256_read_point(q_xy, c, Q);
    p256_load_be(sig, w);
    p256_load_be(sig + 32, ws);
    ok = ok && q256_below_n(w) && q256_below_n(ws);
#pragma unroll
    for (int i = 0; i < 8; ++i) r_words[i] = w[i];
    const Q256 r = q256_from_words_reduced(w), s = q256_from_words_reduced(ws);
    ok = ok && !q256_is_zero(r) && !q256_is_zero(s);
    p256_load_be(digest, w);
    const Q256 d = q256_from_words_reduced(w);
    const Q256 rs_inv = q256_inv(q256_mul(r, s));
    const Q256 s_inv = q256_mul(r, rs_inv), r_inv = q256_mul(s, rs_inv);
    Q256 out[P256_RTU_TERMS];
    out[0] = q256_mul(r, s_inv);
    out[1] = s_inv;
    out[2] = q256_mul(d, s_inv);
    out[3] = q256_mul(d, rs_inv);
    out[4] = q256_neg(q256_mul(d, r_inv));
#pragma unroll
    for (int j = 0; j < P256_RTU_TERMS; ++j) {
        q256_to_words(out[j], w);
#pragma unroll
        for (int i = 0; i < 8; ++i) k[8 * j * stride + i] = w[i];
    }
    return ok;
}

// term t of a row: the first `n_chains` are chains on the row's point, the others walks; tab as p256_chain takes it
CG_HD P256Point p256_term(int t, int n_chains, const P256Affine* __restrict__ g_tab, const P256Affine& pt, const uint32_t* k, P256Point* tab,
                          uint64_t stride, const P256Curve& c) {
    return t < n_chains ? p256_chain(pt, k, tab, stride, c) : p256_walk(g_tab, k, c);
}

// the last stage of compute_TU: both points normalised with one inversion.  T = r^-1 R is never the identity; U is where
// d = 0 mod n, and goes out as 64 zero bytes.
CG_HD void p256_tu_finish(const P256Point& T, const P256Point& U, const P256Curve& c, uint8_t* t_xy, uint8_t* u_xy) {
    const F256 zu = p256_is_identity(U) ? c.one : U.z;
    const F256 inv = f256_inv_hd(f256_mul(T.z, zu));
    uint32_t x[8], y[8];
    p256_affine_words(T, f256_mul(inv, zu), x, y);
    p256_store_be(x, t_xy);
    p256_store_be(y, t_xy + 32);
    p256_affine_words(U, f256_mul(inv, T.z), x, y);
    p256_store_be(x, u_xy);
    p256_store_be(y, u_xy + 32);
}
// the last stage of compute_RTU: part(t) is term t of the row.  R = part(2) + part(0) and T = part(3) + part(1) by the general
// addition; the signature verifies if R is not the identity and R.x mod n = r.  MADE or BAD_SIGNATURE; the caller zeroes a
// row that is not MADE.
template <class Part>
CG_HD uint8_t p256_rtu_finish(Part part, const uint32_t* r_words, const P256Curve& c, uint8_t* r_xy, uint8_t* t_xy, uint8_t* u_xy) {
    const P256Point R = p256_add(part(2), part(0), c), T = p256_add(part(3), part(1), c), U = part(4);
    if (p256_is_identity(R)) return P256_BAD_SIGNATURE;
    const F256 zu = p256_is_identity(U) ? c.one : U.z;
    const F256 z_rt = f256_mul(R.z, T.z);
    const F256 inv = f256_inv_hd(f256_mul(z_rt, zu));
    const F256 inv_rt = f256_mul(inv, zu);                 // (z_R z_T)^-1
    uint32_t x[8], y[8];
    p256_affine_words(R, f256_mul(inv_rt, T.z), x, y);
    uint32_t xr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) xr[i] = x[i];
    q256_reduce_once(xr, 0u);
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) diff |= xr[i] ^ r_words[i];
    if (diff) return P256_BAD_SIGNATURE;
    p256_store_be(x, r_xy);
    p256_store_be(y, r_xy + 32);
    p256_affine_words(T, f256_mul(inv_rt, R.z), x, y);
    p256_store_be(x, t_xy);
    p256_store_be(y, t_xy + 32);
    p256_affine_words(U, f256_mul(inv, z_rt), x, y);
    p256_store_be(x, u_xy);
    p256_store_be(y, u_xy + 32);
    return P256_MADE;
}

// ---- the host's side ------------------------------------------------------------------------------------------------------------
// The table of G: row w entry d - 1 is d·2^(8w)·G.  Additions in projective form, then one inversion for all 8160 points:
// prefix products of the Z, the inverse of the last, and back down.
inline std::vector<P256Affine> p256_make_table() {
    const P256Curve c = p256_curve();
    std::vector<P256Point> pts(P256_TABLE_POINTS);
    P256Point base = p256_from_affine(p256_generator(), c);
    for (int w = 0; w < P256_WINDOWS; ++w) {
        P256Point* row = &pts[(size_t)w * P256_ROW];
        row[0] = base;
        for (int d = 1; d < P256_ROW; ++d) row[d] = p256_add(row[d - 1], base, c);
        base = p256_add(row[P256_ROW - 1], base, c);       // 256 · base
    }
    std::vector<F256> prefix(P256_TABLE_POINTS);
    F256 run = c.one;
    for (int i = 0; i < P256_TABLE_POINTS; ++i) {          // no multiple of G below n is the identity: every Z is non-zero
        prefix[i] = run;
        run = f256_mul(run, pts[i].z);
    }
    F256 inv = f256_inv_hd(run);
    std::vector<P256Affine> tab(P256_TABLE_POINTS);
    for (int i = P256_TABLE_POINTS - 1; i >= 0; --i) {
        const F256 zinv = f256_mul(inv, prefix[i]);
        inv = f256_mul(inv, pts[i].z);
        tab[i] = P256Affine{f256_mul(pts[i].x, zinv), f256_mul(pts[i].y, zinv)};
    }
    return tab;
}
// once per process
inline const std::vector<P256Affine>& p256_table() {
    static const std::vector<P256Affine> t = p256_make_table();
    return t;
}

// whole rows on the host, through the same three stages: the status, and the outputs zero unless it is MADE
inline uint8_t p256_tu_row(const uint8_t* r_xy, const uint8_t* digest, uint8_t* t_xy, uint8_t* u_xy) {
    const P256Curve c = p256_curve();
    P256Affine R;
    uint32_t k[8 * P256_TU_TERMS];
    P256Point tab[P256_CHAIN_TABLE], part[P256_TU_TERMS];
    if (!p256_tu_scalars(r_xy, digest, c, R, k, 1)) {
        p256_zero_bytes(t_xy, 64);
        p256_zero_bytes(u_xy, 64);
        return P256_MALFORMED;
    }
    for (int t = 0; t < P256_TU_TERMS; ++t) part[t] = p256_term(t, P256_TU_CHAINS, p256_table().data(), R, k + 8 * t, tab, 1, c);
    p256_tu_finish(part[0], part[1], c, t_xy, u_xy);
    return P256_MADE;
}
inline uint8_t p256_rtu_row(const uint8_t* q_xy, const uint8_t* sig, const uint8_t* digest, uint8_t* r_xy, uint8_t* t_xy, uint8_t* u_xy) {
    const P256Curve c = p256_curve();
    P256Affine Q;
    uint32_t k[8 * P256_RTU_TERMS], r_words[8];
    P256Point tab[P256_CHAIN_TABLE], part[P256_RTU_TERMS];
    uint8_t status = p256_rtu_scalars(q_xy, sig, digest, c, Q, k, 1, r_words) ? P256_MADE : P256_MALFORMED;
    if (status == P256_MADE) {
        for (int t = 0; t < P256_RTU_TERMS; ++t) part[t] = p256_term(t, P256_RTU_CHAINS, p256_table().data(), Q, k + 8 * t, tab, 1, c);
        status = p256_rtu_finish([&](int t) { return part[t]; }, r_words, c, r_xy, t_xy, u_xy);
    }
    if (status != P256_MADE) {
        p256_zero_bytes(r_xy, 64);
        p256_zero_bytes(t_xy, 64);
        p256_zero_bytes(u_xy, 64);
    }
    return status;
}

}  // namespace cg
