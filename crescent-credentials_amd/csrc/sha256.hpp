// SHA-256 (FIPS 180-4), written once for host and device in the manner of merlin.hpp: what the reference hashes with
// `sha2::Sha256` - the challenge of a device proof (creds/src/device.rs:185-199) and the revealed preimages
// (creds/src/lib.rs:590-603).
//
// The compression function keeps the message schedule as a 16-word window in registers: all 64 rounds are unrolled, so
// every index into the window and every round constant is a constant, and no table lies in memory.  What IS addressed by
// a run-time position is the 64-byte block being filled, which as a per-lane register array would go to scratch.  So it
// is memory the caller names, as merlin.hpp's sponge is: a local array on the host, LDS on the device, SHA_BLOCK bytes
// per lane and 4-byte aligned.  A message is a list of SEGMENTS (bytes behind a pointer, or up to 16 bytes of an immediate,
// or a run of zero bytes) that one loop walks byte by byte with ONE call site of the compression function, so a caller
// never holds a whole message: it names the pieces where they already lie.  The padding is three more segments.
// The kernels built on this declare no private segment (profiles/device_link.md).
#pragma once
#include "merlin.hpp"

namespace cg {

constexpr int SHA_BLOCK = 64;

CG_HD constexpr uint32_t sha_k(int i) {
    constexpr uint32_t k[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
        0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
        0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
        0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
        0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
        0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    return k[i];
}
CG_HD constexpr uint32_t sha_h0(int i) {
    constexpr uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    return h[i];
}
// a rotation by a constant: one funnel shift on the device
CG_HD uint32_t sha_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// One block: h += compress(h, the 16 big-endian words at blk).  Every index below is a constant once the loops are
// unrolled, so the window and the eight working variables are registers.
CG_HD void sha_compress(uint32_t h[8], const uint8_t* blk) {
    const uint32_t* b = (const uint32_t*)blk;
    uint32_t w[16], v[8];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t x = b[i];                                   // the bytes of a word, first byte most significant
        w[i] = (x << 24) | ((x & 0xff00u) << 8) | ((x >> 8) & 0xff00u) | (x >> 24);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = h[i];
#pragma unroll
    for (int t = 0; t < 64; ++t) {
        if (t >= 16) {
            const uint32_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
            const uint32_t s0 = sha_rotr(w15, 7) ^ sha_rotr(w15, 18) ^ (w15 >> 3);
            const uint32_t s1 = sha_rotr(w2, 17) ^ sha_rotr(w2, 19) ^ (w2 >> 10);
            w[t & 15] += s0 + w[(t + 9) & 15] + s1;
        }
        const uint32_t e = v[4], a = v[0];
        const uint32_t t1 = v[7] + (sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25)) + ((e & v[5]) ^ (~e & v[6])) + sha_k(t) + w[t & 15];
        const uint32_t t2 = (sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22)) + ((a & v[1]) ^ (a & v[2]) ^ (v[1] & v[2]));
        v[7] = v[6]; v[6] = v[5]; v[5] = v[4]; v[4] = v[3] + t1;
        v[3] = v[2]; v[2] = v[1]; v[1] = v[0]; v[0] = t1 + t2;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] += v[i];
}

// `len` bytes of a message: behind src, or of lit where src is null (a lit of zeros gives zero bytes at any length)
struct ShaSeg {
    uint32_t len;
    const uint8_t* src;
    MlLit lit;
};
CG_HD ShaSeg sha_bytes(const uint8_t* src, uint32_t len) { return ShaSeg{len, src, MlLit{0, 0, 0}}; }
CG_HD ShaSeg sha_lit(MlLit lit) { return ShaSeg{lit.len, nullptr, lit}; }
CG_HD ShaSeg sha_zeros(uint32_t len) { return ShaSeg{len, nullptr, MlLit{0, 0, 0}}; }

struct Sha256 {
    uint32_t h[8];
    uint8_t* blk;              // SHA_BLOCK bytes, 4-byte aligned
    uint32_t pos;              // bytes of blk filled
    uint64_t total;            // bytes absorbed so far
};
CG_HD Sha256 sha_begin(uint8_t* blk) {
    Sha256 s;
#pragma unroll
    for (int i = 0; i < 8; ++i) s.h[i] = sha_h0(i);
    s.blk = blk;
    s.pos = 0;
    s.total = 0;
    return s;
}

// Absorbs segments seg(0..n), then - where `finish` says so - the padding: 0x80, zeros up to 56 mod 64 and the bit length
// as 8 big-endian bytes, which are segments n .. n + 2 of the same loop.  After a finishing run s.h is the digest's eight
// words.  One step of the inner loop is one byte; the block is compressed where it fills.
template <class SegFn>
CG_HD void sha_run(Sha256& s, int n, bool finish, SegFn seg) {
    const int n_all = finish ? n + 3 : n;
    uint64_t bits = 0;
#pragma nounroll
    for (int i = 0; i < n_all; ++i) {
        ShaSeg g;
        if (i < n) g = seg(i);
        else if (i == n) {
            bits = s.total * 8;
            g = sha_lit(MlLit{0x80, 0, 1});
        } else if (i == n + 1) g = sha_zeros((120u - (uint32_t)(s.total & 63)) & 63u);            // total counts the 0x80 already
        else {
            uint64_t be = 0;
            for (int j = 0; j < 8; ++j) be |= ((bits >> (8 * j)) & 0xffull) << (8 * (7 - j));
            g = sha_lit(MlLit{be, 0, 8});
        }
#pragma nounroll
        for (uint32_t k = 0; k < g.len; ++k) {
            s.blk[s.pos] = g.src ? g.src[k] : (uint8_t)((k < 8 ? g.lit.lo : g.lit.hi) >> (8 * (k & 7)));
            if (++s.pos == SHA_BLOCK) {
                sha_compress(s.h, s.blk);
                s.pos = 0;
            }
        }
        s.total += g.len;
    }
}

// the digest of a finished run as its 32 bytes: word i big-endian at out[4 i ..]
CG_HD void sha_digest(const Sha256& s, uint8_t* out) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) out[4 * i + j] = (uint8_t)(s.h[i] >> (8 * (3 - j)));
}

// SHA-256 of one run of bytes (host and device; blk as above)
CG_HD void sha256_of(uint8_t* blk, const uint8_t* msg, uint64_t len, uint8_t out[32]) {
    Sha256 s = sha_begin(blk);
    sha_run(s, 1, true, [&](int) { return sha_bytes(msg, (uint32_t)len); });
    sha_digest(s, out);
}

}  // namespace cg
