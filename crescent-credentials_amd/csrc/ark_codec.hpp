// What the entries that read and write ark-serialize on the device share (verify.hip, rangeproof.hip, rangeverify.hip):
// the strict host reader of a serialized key, the point codec of the kernels, and `grow` for the device buffers that
// hold no caller's bytes.  The handles' host code - stream, slots, the per-call arrays and their row copies - is in
// key_handle.hpp, which includes this file.
// For .hip files only.
#pragma once
#include "common.hpp"
#include "pairing.hpp"

namespace cg {
namespace {

// ---- strict ark-serialize reader (deserialize_uncompressed_unchecked): canonical coordinates, valid flags --------------
struct KeyRd {
    const uint8_t* p;
    uint64_t len, off;
    void need(uint64_t n) const {
        if (off + n > len || off + n < off) throw HipError(CG_ERR_PARSE, "unexpected end of serialized key");
    }
    uint64_t u64() {
        need(8);
        uint64_t v;
        memcpy(&v, p + off, 8);
        off += 8;
        return v;
    }
    // one field element; `flag_bits` = 0xC0 strips the SWFlags of the coordinate that carries them
    Fq fq(uint8_t flag_bits = 0) {
        need(32);
        uint8_t b[32];
        memcpy(b, p + off, 32);
        b[31] &= (uint8_t)~flag_bits;
        off += 32;
        Fq a = fp_from_bytes<Fq>(b);
        if (!fp_is_canonical(a)) throw HipError(CG_ERR_PARSE, "field element not below the base field modulus");
        return to_mont(a);
    }
    Fq2 fq2(uint8_t flag_bits = 0) {
        Fq c0 = fq();
        Fq c1 = fq(flag_bits);
        return {c0, c1};
    }
    bool flags_infinity(uint64_t last_byte_at) const {
        const uint8_t f = p[last_byte_at] & 0xC0;
        if (f == 0xC0) throw HipError(CG_ERR_PARSE, "invalid point flags");
        return f == 0x40;
    }
    G1Affine g1() {
        need(64);
        const bool inf = flags_infinity(off + 63);
        G1Affine r;
        r.x = fq();
        r.y = fq(0xC0);
        return inf ? G1Affine::inf() : r;
    }
    G2Affine g2() {
        need(128);
        const bool inf = flags_infinity(off + 127);
        G2Affine r;
        r.x = fq2();
        r.y = fq2(0xC0);
        return inf ? G2Affine::inf() : r;
    }
    uint64_t count(uint64_t item_bytes) {
        uint64_t n = u64();
        if (n > (len - off) / item_bytes) throw HipError(CG_ERR_PARSE, "vector length exceeds the remaining data");
        return n;
    }
};

// ark's checked deserialisation of one uncompressed G1 point on the host (the Pedersen bases a range proof key registers):
// flags, coordinates < q, the curve equation (G1 has cofactor 1)
[[maybe_unused]] bool checked_g1(const uint8_t* b, G1Affine& p) {
    const uint8_t f = b[63] & 0xC0;
    if (f == 0xC0) return false;
    uint8_t yb[32];
    memcpy(yb, b + 32, 32);
    yb[31] &= 0x3F;
    const Fq x = fp_from_bytes<Fq>(b), y = fp_from_bytes<Fq>(yb);
    if (!fp_is_canonical(x) || !fp_is_canonical(y)) return false;
    if (f == 0x40) { p = G1Affine::inf(); return true; }
    p = {to_mont(x), to_mont(y)};
    return g1_on_curve(p);
}

// ---- device side: ark-serialize points, read (checked, or unchecked for the chains) and written ---------------------------
__device__ __forceinline__ bool limbs_below(const uint32_t a[8], const uint32_t n[8]) {
    for (int i = 7; i >= 0; --i) {
        if (a[i] < n[i]) return true;
        if (a[i] > n[i]) return false;
    }
    return false;
}
// one coordinate from 8 words; strip = the SWFlags bits of the word that carries them
__device__ __forceinline__ Fq dev_fq(const uint32_t* w, bool& ok, uint32_t strip = 0) {
    uint32_t l[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) l[i] = w[i];
    l[7] &= ~strip;
    ok = ok && limbs_below(l, FqP::N);
    Fq a;
#pragma unroll
    for (int i = 0; i < 8; ++i) a.l[i] = l[i];
    return to_mont(a);
}
// checked deserialisation of one uncompressed G1 point (16 words): flags valid, coordinates < q, on the curve unless O
__device__ __forceinline__ G1Affine dev_g1(const uint32_t* w, bool& ok) {
    const uint32_t f = w[15] >> 30;
    ok = ok && f != 3u;
    G1Affine p;
    p.x = dev_fq(w, ok);
    p.y = dev_fq(w + 8, ok, 0xC0000000u);
    if (f == 1u) return G1Affine::inf();
    ok = ok && g1_on_curve(p);
    return p;
}
// SUBGROUP = false stops at the twist equation (a client state's own proof, cg_show_commit_batch)
template <bool SUBGROUP = true>
__device__ __forceinline__ G2Affine dev_g2(const uint32_t* w, bool& ok) {
    const uint32_t f = w[31] >> 30;
    ok = ok && f != 3u;
    G2Affine p;
    p.x.c0 = dev_fq(w, ok);
    p.x.c1 = dev_fq(w + 8, ok);
    p.y.c0 = dev_fq(w + 16, ok);
    p.y.c1 = dev_fq(w + 24, ok, 0xC0000000u);
    if (f == 1u) return G2Affine::inf();
    ok = ok && g2_on_twist(p);
    if (SUBGROUP && ok) ok = g2_in_subgroup(p);
    return p;
}

// the same points as the chains use them: no checks (k_show_check / k_mk_check make them, and an item that fails them has
// its output zeroed), flags stripped
__device__ __forceinline__ G1Affine dev_g1_unchecked(const uint32_t* w) {
    if ((w[15] >> 30) == 1u) return G1Affine::inf();
    bool ignored = true;
    G1Affine p;
    p.x = dev_fq(w, ignored);
    p.y = dev_fq(w + 8, ignored, 0xC0000000u);
    return p;
}
__device__ __forceinline__ G2Affine dev_g2_unchecked(const uint32_t* w) {
    if ((w[31] >> 30) == 1u) return G2Affine::inf();
    bool ignored = true;
    G2Affine p;
    p.x.c0 = dev_fq(w, ignored);
    p.x.c1 = dev_fq(w + 8, ignored);
    p.y.c0 = dev_fq(w + 16, ignored);
    p.y.c1 = dev_fq(w + 24, ignored, 0xC0000000u);
    return p;
}
// ark-serialize of an affine G1 point: uncompressed (16 words) or compressed (8 words), SWFlags in the top bits
__device__ __forceinline__ void dev_put_g1(const G1Affine& a, uint32_t* out, bool compressed) {
    Fq x = Fq::zero(), y = Fq::zero();
    uint32_t flags = 0x40000000u;                                 // SWFlags::PointAtInfinity
    if (!a.is_inf()) {
        x = from_mont(a.x);
        y = from_mont(a.y);
        const Fq ny = from_mont(neg(a.y));
        flags = limbs_below(ny.l, y.l) ? 0x80000000u : 0u;        // SWFlags::YIsNegative: y > -y
    }
    (compressed ? x : y).l[7] |= flags;
#pragma unroll
    for (int l = 0; l < 8; ++l) out[l] = x.l[l];
    if (!compressed) {
#pragma unroll
        for (int l = 0; l < 8; ++l) out[8 + l] = y.l[l];
    }
}
__device__ __forceinline__ void dev_put_g2(const G2Affine& a, uint32_t* out) {
    if (a.is_inf()) {
        for (int l = 0; l < 32; ++l) out[l] = l == 31 ? 0x40000000u : 0u;
        return;
    }
    const Fq2 ny = neg(a.y);
    const Fq c[4] = {from_mont(a.x.c0), from_mont(a.x.c1), from_mont(a.y.c0), from_mont(a.y.c1)};
    const Fq n0 = from_mont(ny.c0), n1 = from_mont(ny.c1);
    for (int j = 0; j < 4; ++j)
        for (int l = 0; l < 8; ++l) out[8 * j + l] = c[j].l[l];
    // QuadExtField's ordering compares c1 first, then c0
    const bool larger = c[3] == n1 ? limbs_below(n0.l, c[2].l) : limbs_below(n1.l, c[3].l);
    if (larger) out[31] |= 0x80000000u;
}

__device__ __forceinline__ Fr dev_fr(const uint32_t* w) {
    Fr a;
#pragma unroll
    for (int i = 0; i < 8; ++i) a.l[i] = w[i];
    return a;
}

template <class T>
static void grow(DevBuf<T>& b, uint64_t count) {
    if (b.n < count) b.alloc(count);
}

}  // namespace
}  // namespace cg
