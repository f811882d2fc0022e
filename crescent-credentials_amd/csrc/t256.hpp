// The group T-256 (forks/halo2curves/src/t256/curve.rs:35-59): y^2 = x^3 - 3x + b over ft256.hpp's field, with
//     b = 0x b441071b12f4a036 6fb552f8e21ed4ac 36b06aceeb354224 863e60f20219fc56,
//     G = (5, 0x 3e86c0cfebf2c716 5efc7b55f6b24fbe 0ed60b9e33ce397c 5826108a653de28d),
// of prime order q = P-256's base prime, so that its scalar field is fp256.hpp's; written once for host and device.  Every
// commitment of `spartan_t256` lives in it: a Pedersen vector commitment sum_j z_j G_j + blind h (`Vec<Scalar>::commit`,
// forks/Spartan-t256/src/commitments.rs:81-99) and, one per row of the witness matrix, the Hyrax commitment of
// `DensePolynomial::commit` (dense_mlpoly.rs:151-206).  tests/t256_vectors.py asserts a = -3, G on the curve and q·G = O.
//
// Coordinates and formulas are p256.hpp's, restated over the other field with the other b: homogeneous projective (X : Y : Z),
// the identity (0 : 1 : 0), the COMPLETE addition of Renes, Costello and Batina (Eurocrypt 2016, section 3) for a = -3.  With
//     xx = X1 X2, yy = Y1 Y2, zz = Z1 Z2, xy = X1 Y2 + X2 Y1, xz = X1 Z2 + X2 Z1, yz = Y1 Z2 + Y2 Z1,
//     A = 3 (b zz - xz), B = 3 (b xz - xx - 3 zz), C = 3 (xx - zz)
// the sum is X3 = xy (yy - A) - yz B, Y3 = (yy + A)(yy - A) + C B, Z3 = yz (yy + A) + xy C: twelve products and two by b; the
// mixed addition (Z2 = 1) eleven and two.  The order is an odd prime, so the formula has no exceptional pair - P + P, P + (-P),
// P + O and O + O go through the same straight line - and an 8-bit table entry d·2^(8w)·P of a point P != O is never the
// identity.  That matters here: a caller's generators may repeat or be opposite, and partial sums of a row then coincide or
// cancel where they meet.
//
// Bytes (halo2curves; each reading is restated, not copied, and UNVERIFIED in the sense of DESIGN.md 3 - the reference pins no
// T-256 bytes, curve.rs:129 says so itself - so each form has ONE reader or writer here and one in tests/t256_vectors.py):
//   a coordinate      32 B big-endian: the field is declared `endian = "big"` (t256/fp.rs; derive/src/field/mod.rs:326-344)
//   a scalar          32 B little-endian (t256/fq.rs:14; derive/src/field/mod.rs:470-476), the form
//                     cg_poseidon_p256_permute_batch takes for the same field
//   uncompressed      x ‖ y, 64 B; the identity is 64 zero bytes (src/derive/curve.rs:139-181, serde.rs:174-319)
//   compressed        33 B, `CompressedFlagConfig::Extra` (src/derive/curve.rs:69-73): byte 0 the flags - bit 7 set when y is
//                     odd (`to_repr` is little-endian whatever the field's `endian`, so `to_repr()[0] & 1` is the parity), bit 6
//                     set for the identity, whose parity bit is clear - then x big-endian; the identity is 0x40 and 32 zero bytes
//
// Fixed bases: fixed_base.hpp's geometry - 8-bit windows, 32 rows of 255 affine points per base, row w entry d - 1 being
// d·2^(8w)·P, 64 B a point, 522 240 B a base - built on the host by additions and one batched inversion per base, as
// p256_make_table builds G's.  A scalar costs as many mixed additions as it has non-zero bytes: a 0 wire none, a 1 wire one.
// ONE walk serves host and device: t256_walk_share runs one lane's share of a row's digits into a projective partial.
// Scalars are read through pointers to canonical words in memory, never out of a per-lane array indexed by a run-time value:
// the kernels that inline this declare no private segment.  Constant time is not a requirement of the walk's shape; it skips
// zero digits.
#pragma once
#include <vector>

#include "fp256.hpp"
#include "ft256.hpp"

namespace cg {

struct T256Affine {
    FT256 x, y;                            // Montgomery form; never the identity
};
struct T256Point {
    FT256 x, y, z;                         // (X : Y : Z), Montgomery form; the identity is (0 : 1 : 0)
};
// what the formulas need of the curve, in Montgomery form: b and 1
struct T256Curve {
    FT256 b, one;
};

constexpr int T256_WINDOWS = 32, T256_ROW = 255;
constexpr int T256_TABLE_POINTS = T256_WINDOWS * T256_ROW;
constexpr int T256_COMPRESSED = 33;
enum : uint8_t { T256_MADE = 1, T256_MALFORMED = 2 };                              // CG_SHOW_MADE, CG_SHOW_MALFORMED
enum : int { T256_GENS_OK = 0, T256_GENS_NOT_CANONICAL = 1, T256_GENS_OFF_CURVE = 2, T256_GENS_IDENTITY = 3 };

CG_HD constexpr uint32_t t256_b(int i) {
    constexpr uint32_t b[8] = {0x0219fc56u, 0x863e60f2u, 0xeb354224u, 0x36b06aceu, 0xe21ed4acu, 0x6fb552f8u, 0x12f4a036u, 0xb441071bu};
    return b[i];
}
CG_HD constexpr uint32_t t256_gx(int i) { return i == 0 ? 5u : 0u; }
CG_HD constexpr uint32_t t256_gy(int i) {
    constexpr uint32_t y[8] = {0x653de28du, 0x5826108au, 0x33ce397cu, 0x0ed60b9eu, 0xf6b24fbeu, 0x5efc7b55u, 0xebf2c716u, 0x3e86c0cfu};
    return y[i];
}

CG_HD T256Curve t256_curve() {
    T256Curve c;
    FT256 b, one = ft256_zero();
#pragma unroll
    for (int i = 0; i < 8; ++i) b.l[i] = t256_b(i);
    one.l[0] = 1;
    c.b = ft256_to_mont(b);
    c.one = ft256_to_mont(one);
    return c;
}
CG_HD T256Point t256_identity(const T256Curve& c) { return T256Point{ft256_zero(), c.one, ft256_zero()}; }
CG_HD bool t256_is_identity(const T256Point& p) { return ft256_is_zero(p.z); }
CG_HD T256Point t256_from_affine(const T256Affine& a, const T256Curve& c) { return T256Point{a.x, a.y, c.one}; }
CG_HD T256Affine t256_neg(const T256Affine& a) { return T256Affine{a.x, ft256_neg(a.y)}; }
CG_HD T256Affine t256_generator() {
    FT256 x, y;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        x.l[i] = t256_gx(i);
        y.l[i] = t256_gy(i);
    }
    return T256Affine{ft256_to_mont(x), ft256_to_mont(y)};
}
CG_HD FT256 ft256_triple(const FT256& a) { return ft256_add(ft256_add(a, a), a); }
// y^2 = x^3 - 3x + b
CG_HD bool t256_on_curve(const T256Affine& a, const T256Curve& c) {
    const FT256 rhs = ft256_add(ft256_sub(ft256_mul(ft256_sqr(a.x), a.x), ft256_triple(a.x)), c.b);
    return ft256_eq(ft256_sqr(a.y), rhs);
}

// the second half of both additions: the header has the formula
CG_HD T256Point t256_add_tail(const FT256& xx, const FT256& yy, const FT256& zz, const FT256& xy, const FT256& xz, const FT256& yz,
                              const T256Curve& c) {
    const FT256 A = ft256_triple(ft256_sub(ft256_mul(c.b, zz), xz));
    const FT256 B = ft256_triple(ft256_sub(ft256_sub(ft256_mul(c.b, xz), xx), ft256_triple(zz)));
    const FT256 C = ft256_triple(ft256_sub(xx, zz));
    const FT256 lo = ft256_sub(yy, A), up = ft256_add(yy, A);
    T256Point r;
    r.x = ft256_sub(ft256_mul(xy, lo), ft256_mul(yz, B));
    r.y = ft256_add(ft256_mul(up, lo), ft256_mul(C, B));
    r.z = ft256_add(ft256_mul(yz, up), ft256_mul(xy, C));
    return r;
}
// the general, complete addition: any two points of the group, equal, opposite or the identity
CG_HD T256Point t256_add(const T256Point& p, const T256Point& q, const T256Curve& c) {
    const FT256 xx = ft256_mul(p.x, q.x), yy = ft256_mul(p.y, q.y), zz = ft256_mul(p.z, q.z);
    const FT256 xy = ft256_sub(ft256_sub(ft256_mul(ft256_add(p.x, p.y), ft256_add(q.x, q.y)), xx), yy);
    const FT256 xz = ft256_sub(ft256_sub(ft256_mul(ft256_add(p.x, p.z), ft256_add(q.x, q.z)), xx), zz);
    const FT256 yz = ft256_sub(ft256_sub(ft256_mul(ft256_add(p.y, p.z), ft256_add(q.y, q.z)), yy), zz);
    return t256_add_tail(xx, yy, zz, xy, xz, yz, c);
}
CG_HD T256Point t256_double(const T256Point& p, const T256Curve& c) { return t256_add(p, p, c); }
// the same against an affine point (Z2 = 1), complete for every p, the identity included
CG_HD T256Point t256_add_mixed(const T256Point& p, const T256Affine& q, const T256Curve& c) {
    const FT256 xx = ft256_mul(p.x, q.x), yy = ft256_mul(p.y, q.y);
    const FT256 xy = ft256_sub(ft256_sub(ft256_mul(ft256_add(p.x, p.y), ft256_add(q.x, q.y)), xx), yy);
    const FT256 xz = ft256_add(p.x, ft256_mul(q.x, p.z));
    const FT256 yz = ft256_add(p.y, ft256_mul(q.y, p.z));
    return t256_add_tail(xx, yy, p.z, xy, xz, yz, c);
}

// ---- bytes --------------------------------------------------------------------------------------------------------------------
// a coordinate: 32 bytes big-endian <-> eight words
CG_HD void t256_load_be(const uint8_t* b, uint32_t w[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
        w[i] = (uint32_t)b[31 - 4 * i] | ((uint32_t)b[30 - 4 * i] << 8) | ((uint32_t)b[29 - 4 * i] << 16) | ((uint32_t)b[28 - 4 * i] << 24);
}
CG_HD void t256_store_be(const uint32_t w[8], uint8_t* b) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        b[31 - 4 * i] = (uint8_t)w[i];
        b[30 - 4 * i] = (uint8_t)(w[i] >> 8);
        b[29 - 4 * i] = (uint8_t)(w[i] >> 16);
        b[28 - 4 * i] = (uint8_t)(w[i] >> 24);
    }
}
// a scalar: 32 bytes little-endian -> eight words (on the device a scalar array IS its words; the host's callers hand over
// bytes of any alignment)
CG_HD void t256_load_scalar(const uint8_t* b, uint32_t w[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
        w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
}
// the eight words are a scalar: below q, the base prime of P-256
CG_HD bool t256_scalar_ok(const uint32_t* w) { return f256_below_p(w); }

// THE reader of the uncompressed form: x ‖ y, 64 bytes -> the point.  T256_GENS_IDENTITY for 64 zero bytes,
// T256_GENS_NOT_CANONICAL if a coordinate is >= p_T (the reference reduces it silently; this project fails closed on
// non-canonical input), T256_GENS_OFF_CURVE if the point is not on the curve.
CG_HD int t256_read_point(const uint8_t* xy, const T256Curve& c, T256Affine& out) {
    uint32_t x[8], y[8], any = 0;
    t256_load_be(xy, x);
    t256_load_be(xy + 32, y);
#pragma unroll
    for (int i = 0; i < 8; ++i) any |= x[i] | y[i];
    if (!any) return T256_GENS_IDENTITY;
    if (!ft256_below_p(x) || !ft256_below_p(y)) return T256_GENS_NOT_CANONICAL;
    out.x = ft256_from_words(x);
    out.y = ft256_from_words(y);
    return t256_on_curve(out, c) ? T256_GENS_OK : T256_GENS_OFF_CURVE;
}
// THE writer of the compressed form: (X : Y : Z) with Z^-1 given (anything for the identity) -> 33 bytes
CG_HD void t256_write_compressed(const T256Point& p, const FT256& zinv, uint8_t* out) {
    if (t256_is_identity(p)) {
        out[0] = 0x40;
        for (int i = 1; i < T256_COMPRESSED; ++i) out[i] = 0;
        return;
    }
    uint32_t x[8], y[8];
    ft256_to_words(ft256_mul(p.x, zinv), x);
    ft256_to_words(ft256_mul(p.y, zinv), y);
    out[0] = (uint8_t)((y[0] & 1u) << 7);
    t256_store_be(x, out + 1);
}
// the uncompressed form, for the tests' view of the arithmetic: the identity is 64 zero bytes
CG_HD void t256_write_uncompressed(const T256Point& p, const FT256& zinv, uint8_t* out) {
    uint32_t x[8], y[8];
    const bool inf = t256_is_identity(p);
    ft256_to_words(ft256_mul(p.x, zinv), x);
    ft256_to_words(ft256_mul(p.y, zinv), y);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        x[i] = inf ? 0u : x[i];
        y[i] = inf ? 0u : y[i];
    }
    t256_store_be(x, out);
    t256_store_be(y, out + 32);
}

// ---- the walk -------------------------------------------------------------------------------------------------------------------
// Lane t's share of one row, t < W = 2^log_w <= 64, summed into a projective partial; the W shares make the row.  Term j < n_gens
// is srow[8 j ..] · G_j, term n_gens is blind · h; the table of term j starts at tabs + j · T256_TABLE_POINTS.  Scalars are
// canonical words IN MEMORY (any 256-bit integer would do: the table covers them all).
// The share is cut by DIGIT, not by term: of term j the lane takes the windows w = (t - j) mod W, + W, + 2W, ... below 32.  A
// wide scalar's 32 digits so spread over min(W, 32) lanes, and window 0 - the only digit of a wire that is 1 - falls to lane
// j mod W.  Cut by term, a circuit's mix of wires (most 0 or 1, a tenth wide) left a wave waiting for the lane that drew the
// most wide scalars: 4.8 times the time per addition of uniform rows, measured (profiles/t256_commit.md).  The host walks a
// whole row as the one lane of W = 1.
// The scan takes four of the lane's digits at a time, their loads in flight together, and the addition follows the first that
// is not zero: the lanes of a wave meet at the addition with a digit each, so a lane's cost is its count of non-zero digits.
CG_HD uint32_t t256_share_digit(const uint32_t* srow, const uint32_t* blind, uint32_t n_gens, uint32_t t, uint32_t log_w, uint32_t log_per, uint32_t i,
                                uint32_t end, uint64_t* at) {
    if (i >= end) return 0;
    const uint32_t W = 1u << log_w, j = i >> log_per, r = i & ((1u << log_per) - 1);
    const uint32_t w = ((t + W - (j & (W - 1))) & (W - 1)) + (r << log_w);
    if (w >= (uint32_t)T256_WINDOWS) return 0;                                  // W = 64: every other term has no window for this lane
    const uint32_t* k = j < n_gens ? srow + 8 * (uint64_t)j : blind;
    const uint32_t d = (k[w >> 2] >> (8 * (w & 3u))) & 255u;
    *at = ((uint64_t)j * T256_WINDOWS + w) * T256_ROW + d - 1;                  // read only where d is not zero
    return d;
}
CG_HD T256Point t256_walk_share(const T256Affine* __restrict__ tabs, const uint32_t* srow, const uint32_t* blind, uint32_t n_gens, uint32_t t,
                                uint32_t log_w, const T256Curve& c) {
    T256Point acc = t256_identity(c);
    const uint32_t log_per = log_w >= 5 ? 0u : 5u - log_w;                      // the lane has 2^log_per windows of one term
    const uint32_t end = (n_gens + 1) << log_per;                              // below 2^17: a set has at most 2056 tables
    uint32_t i = 0;
#pragma unroll 1
    for (;;) {
        uint32_t d = 0;
        uint64_t at = 0;
#pragma unroll 1
        while (i < end) {
            uint64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
            const uint32_t d0 = t256_share_digit(srow, blind, n_gens, t, log_w, log_per, i, end, &a0);
            const uint32_t d1 = t256_share_digit(srow, blind, n_gens, t, log_w, log_per, i + 1, end, &a1);
            const uint32_t d2 = t256_share_digit(srow, blind, n_gens, t, log_w, log_per, i + 2, end, &a2);
            const uint32_t d3 = t256_share_digit(srow, blind, n_gens, t, log_w, log_per, i + 3, end, &a3);
            if (!(d0 | d1 | d2 | d3)) {
                i += 4;
                continue;
            }
            d = d0 ? d0 : d1 ? d1 : d2 ? d2 : d3;
            at = d0 ? a0 : d1 ? a1 : d2 ? a2 : a3;
            i += d0 ? 1 : d1 ? 2 : d2 ? 3 : 4;
            break;
        }
        if (!d) break;
        acc = t256_add_mixed(acc, tabs[at], c);
    }
    return acc;
}

// ---- the host's side ------------------------------------------------------------------------------------------------------------
// The table of one base: row w entry d - 1 is d·2^(8w)·P.  Additions in projective form, then one inversion for all 8160
// points: prefix products of the Z, the inverse of the last, and back down.  P is not the identity and the order is prime, so
// no entry is the identity and every Z is non-zero.
inline void t256_make_table(const T256Affine& p, T256Affine* tab) {
    const T256Curve c = t256_curve();
    std::vector<T256Point> pts(T256_TABLE_POINTS);
    T256Point base = t256_from_affine(p, c);
    for (int w = 0; w < T256_WINDOWS; ++w) {
        T256Point* row = &pts[(size_t)w * T256_ROW];
        row[0] = base;
        for (int d = 1; d < T256_ROW; ++d) row[d] = t256_add(row[d - 1], base, c);
        base = t256_add(row[T256_ROW - 1], base, c);       // 256 · base
    }
    std::vector<FT256> prefix(T256_TABLE_POINTS);
    FT256 run = c.one;
    for (int i = 0; i < T256_TABLE_POINTS; ++i) {
        prefix[i] = run;
        run = ft256_mul(run, pts[i].z);
    }
    FT256 inv = ft256_inv(run);
    for (int i = T256_TABLE_POINTS - 1; i >= 0; --i) {
        const FT256 zinv = ft256_mul(inv, prefix[i]);
        inv = ft256_mul(inv, pts[i].z);
        tab[i] = T256Affine{ft256_mul(pts[i].x, zinv), ft256_mul(pts[i].y, zinv)};
    }
}

// `MultiCommitGens { G, h }` as uncompressed points -> the n_gens + 1 points in table order (h last), or the first refusal:
// its code, and in *which the index of the point (n_gens for h).  What cg_t256_gens_load runs before any HIP call.
inline int t256_read_gens(const uint8_t* g_xy, uint64_t n_gens, const uint8_t* h_xy, std::vector<T256Affine>& out, uint64_t* which) {
    const T256Curve c = t256_curve();
    out.resize(n_gens + 1);
    for (uint64_t j = 0; j <= n_gens; ++j) {
        const int rc = t256_read_point(j < n_gens ? g_xy + 64 * j : h_xy, c, out[j]);
        if (rc != T256_GENS_OK) {
            *which = j;
            return rc;
        }
    }
    return T256_GENS_OK;
}

// One row on the host, through the device's walk: sum_j scalars[j] · G_j + blind · h, compressed.  T256_MALFORMED, and 33
// zero bytes, where a scalar or the blind is >= q.
inline uint8_t t256_commit_row(const T256Affine* tabs, uint64_t n_gens, const uint8_t* scalars, const uint8_t* blind, uint8_t* out33) {
    const T256Curve c = t256_curve();
    std::vector<uint32_t> k(8 * (n_gens + 1));
    bool ok = true;
    for (uint64_t j = 0; j <= n_gens; ++j) {
        t256_load_scalar(j < n_gens ? scalars + 32 * j : blind, &k[8 * j]);
        ok = ok && t256_scalar_ok(&k[8 * j]);
    }
    if (!ok) {
        for (int i = 0; i < T256_COMPRESSED; ++i) out33[i] = 0;
        return T256_MALFORMED;
    }
    const T256Point sum = t256_walk_share(tabs, k.data(), &k[8 * n_gens], (uint32_t)n_gens, 0, 0, c);
    t256_write_compressed(sum, ft256_inv(sum.z), out33);
    return T256_MADE;
}

}  // namespace cg
