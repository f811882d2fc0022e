// Merlin transcripts as the `merlin` crate (v3) computes them - STROBE-128 cut down to meta-AD, AD and PRF over
// Keccak-f[1600] - and the two transcript shapes the reference builds on them (creds/src/utils.rs:29-37):
//   range     com_f, com_g -> c; com_q -> rho                                   (creds/src/rangeproof.rs:250-274, 352-366)
//   DLogPoK   context, then per statement its bases, k and y -> c               (creds/src/dlog.rs:56-58, 77-99, 130-169)
//             as the fixed shape of a range proof's DLEQ, and for any shape (ml_dlog_shape_challenge: a showing's)
// Every message is the value's ark-serialize COMPRESSED bytes, every transcript is Transcript::new(&[0u8]) and every
// challenge 31 bytes under the label [0u8], read little-endian: a canonical scalar whose top byte is 0.
//
// Written once for host and device.  The sponge is 200 bytes addressed by a run-time position, which as a per-lane
// register array would go to scratch.  So it is memory the caller names: a local array on the host, LDS on the device,
// 200 bytes per lane (ML_STATE), read into 25 registers for the permutation and written back.  A transcript is a list of
// SEGMENTS (one STROBE operation each: its two header bytes, then its bytes absorbed or squeezed) that one loop walks
// byte by byte, so that the permutation - fully unrolled, 64-bit lanes - has ONE call site per transcript however many
// operations it has.  Labels and lengths are immediates (up to 16 bytes in two words), not pointers: a kernel takes no
// address of a constant.  The kernels built on this declare no private segment (tests/test_transcript_cpu.py).
#pragma once
#include "field.hpp"

namespace cg {

constexpr int ML_STATE = 200;              // bytes of sponge per transcript, 8-byte aligned
constexpr int ML_RATE = 166;               // STROBE-128: 200 - 128/4 - 2
constexpr int ML_CHALLENGE = 31;           // bytes drawn per challenge (utils.rs: from_random_bytes of 31)
enum { ML_I = 1, ML_A = 2, ML_C = 4, ML_T = 8, ML_M = 16, ML_K = 32 };
enum { ML_META_AD = ML_M | ML_A, ML_AD = ML_A, ML_PRF = ML_I | ML_A | ML_C };

CG_HD constexpr uint64_t ml_round_constant(int i) {
    constexpr uint64_t rc[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
                                 0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
                                 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
                                 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
                                 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
                                 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    return rc[i];
}
CG_HD constexpr int ml_rho_offset(int i) {             // of lane x + 5y
    constexpr int r[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
    return r[i];
}
// a rotation by a constant: two 32-bit funnel shifts on the device
CG_HD uint64_t ml_rotl(uint64_t x, int n) { return n ? (x << n) | (x >> (64 - n)) : x; }

// Keccak-f[1600] on the 25 little-endian lanes at st.  Every index below is a constant once the loops are unrolled, so
// the lanes are registers.
CG_HD void ml_keccak_f(uint8_t* st) {
    uint64_t* s = (uint64_t*)st;
    uint64_t a[25], b[25], c[5];
#pragma unroll
    for (int i = 0; i < 25; ++i) a[i] = s[i];
#pragma unroll
    for (int round = 0; round < 24; ++round) {
#pragma unroll
        for (int x = 0; x < 5; ++x) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; ++x) {
            const uint64_t d = c[(x + 4) % 5] ^ ml_rotl(c[(x + 1) % 5], 1);
#pragma unroll
            for (int y = 0; y < 5; ++y) a[x + 5 * y] ^= d;
        }
#pragma unroll
        for (int x = 0; x < 5; ++x)
#pragma unroll
            for (int y = 0; y < 5; ++y) b[y + 5 * ((2 * x + 3 * y) % 5)] = ml_rotl(a[x + 5 * y], ml_rho_offset(x + 5 * y));
#pragma unroll
        for (int x = 0; x < 5; ++x)
#pragma unroll
            for (int y = 0; y < 5; ++y) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        a[0] ^= ml_round_constant(round);
    }
#pragma unroll
    for (int i = 0; i < 25; ++i) s[i] = a[i];
}

// up to 16 bytes as two little-endian words: a label, a length, a usize
struct MlLit {
    uint64_t lo, hi;
    uint32_t len;
};
template <int N>
CG_HD constexpr MlLit ml_lit(const char (&s)[N]) {     // a string literal without its terminator
    MlLit l{0, 0, (uint32_t)(N - 1)};
    for (int i = 0; i < N - 1; ++i) {
        if (i < 8) l.lo |= (uint64_t)(uint8_t)s[i] << (8 * i);
        else l.hi |= (uint64_t)(uint8_t)s[i] << (8 * (i - 8));
    }
    return l;
}
CG_HD constexpr MlLit ml_u32(uint32_t v) { return MlLit{v, 0, 4}; }
CG_HD constexpr MlLit ml_u64(uint64_t v) { return MlLit{v, 0, 8}; }
CG_HD constexpr MlLit ml_zero_byte() { return MlLit{0, 0, 1}; }                  // the label and the dom-sep &[0u8]

// One STROBE operation.  Its bytes come from src, or from lit where src is null; a PRF writes them to dst (null: drawn
// and dropped, as when a transcript is replayed up to a later challenge).
struct MlSeg {
    uint8_t flags;
    bool more;                 // continues the operation before it: no header
    uint32_t len;
    const uint8_t* src;
    MlLit lit;
    uint8_t* dst;
};

struct Strobe {
    uint8_t* st;               // ML_STATE bytes
    uint32_t pos, pos_begin, cur_flags;
    bool fresh;                // nothing run yet: the first ml_run initialises the sponge
};
CG_HD Strobe ml_strobe(uint8_t* st) { return Strobe{st, 0, 0, 0, true}; }

// Runs segments seg(0..n) on s.  One step of the loop is one byte (a header byte, a byte absorbed or a byte squeezed) or
// the forced run_f of an operation with C or K; the permutation is at the loop's head, pending from the step before.
template <class SegFn>
CG_HD void ml_run(Strobe& s, int n, SegFn seg) {
    bool f = false, raw = false;
    int first = 0;
    if (s.fresh) {             // STROBE-128/1600 init: the permutation of the domain string, then meta-AD "Merlin v1.0"
        for (int i = 0; i < ML_STATE; ++i) s.st[i] = 0;
        const MlLit head = {0x60010001a801ull, 0, 6};                                  // 01 A8 01 00 01 60
        const MlLit name = ml_lit("STROBEv1.0.2");
        for (int i = 0; i < 6; ++i) s.st[i] = (uint8_t)(head.lo >> (8 * i));
        for (int i = 0; i < 12; ++i) s.st[6 + i] = (uint8_t)((i < 8 ? name.lo >> (8 * i) : name.hi >> (8 * (i - 8))));
        s.pos = s.pos_begin = s.cur_flags = 0;
        s.fresh = false;
        f = raw = true;
        first = -1;
    }
#pragma nounroll
    for (int i = first; i < n; ++i) {
        const MlSeg g = i < 0 ? MlSeg{ML_META_AD, false, 11, nullptr, ml_lit("Merlin v1.0"), nullptr} : seg(i);
        const int header = g.more ? 0 : 3;
        uint32_t old_begin = 0;
#pragma nounroll
        for (int k = -header; k < (int)g.len || f; ++k) {
            if (f) {
                if (!raw) {    // run_f
                    s.st[s.pos] ^= (uint8_t)s.pos_begin;
                    s.st[s.pos + 1] ^= 0x04;
                    s.st[ML_RATE + 1] ^= 0x80;
                }
                ml_keccak_f(s.st);
                s.pos = s.pos_begin = 0;
                f = raw = false;
                if (k >= (int)g.len) break;
            }
            if (k == -1) {     // begin_op's end: an operation with C or K starts on a fresh block
                f = (g.flags & (ML_C | ML_K)) && s.pos != 0;
                continue;
            }
            if (k == -3) {     // begin_op
                old_begin = s.pos_begin;
                s.pos_begin = s.pos + 1;
                s.cur_flags = g.flags;
            }
            if (k < 0 || g.flags != ML_PRF) {
                uint8_t b;
                if (k == -3) b = (uint8_t)old_begin;
                else if (k == -2) b = g.flags;
                else if (g.src) b = g.src[k];
                else b = (uint8_t)((k < 8 ? g.lit.lo : g.lit.hi) >> (8 * (k & 7)));
                s.st[s.pos] ^= b;
            } else {
                if (g.dst) g.dst[k] = s.st[s.pos];
                s.st[s.pos] = 0;
            }
            f = ++s.pos == ML_RATE;
        }
    }
}

// A transcript's calls after Transcript::new(&[0u8]): append_message(label, msg) or challenge_bytes(label, n) -> dst
struct MlItem {
    MlLit label;
    bool challenge;
    uint32_t len;              // of the message, or bytes drawn
    const uint8_t* msg;        // null: the message is `lit`
    MlLit lit;
    uint8_t* dst;
};
CG_HD MlItem ml_append(MlLit label, const uint8_t* msg, uint32_t len) { return MlItem{label, false, len, msg, MlLit{0, 0, 0}, nullptr}; }
CG_HD MlItem ml_append(MlLit label, MlLit msg) { return MlItem{label, false, msg.len, nullptr, msg, nullptr}; }
CG_HD MlItem ml_challenge(uint8_t* dst) { return MlItem{ml_zero_byte(), true, ML_CHALLENGE, nullptr, MlLit{0, 0, 0}, dst}; }

// the three STROBE operations of item `it`: meta-AD(label), meta-AD(u32le(len), more), then AD(msg) or PRF(len)
CG_HD MlSeg ml_item_seg(const MlItem& it, int part) {
    if (part == 0) return MlSeg{ML_META_AD, false, it.label.len, nullptr, it.label, nullptr};
    if (part == 1) return MlSeg{ML_META_AD, true, 4, nullptr, ml_u32(it.len), nullptr};
    return MlSeg{(uint8_t)(it.challenge ? ML_PRF : ML_AD), false, it.len, it.msg, it.lit, it.dst};
}

// Transcript::new(&[0u8]) and items item(0..n) on the sponge at st
template <class ItemFn>
CG_HD void ml_transcript(uint8_t* st, int n, ItemFn item) {
    Strobe s = ml_strobe(st);
    ml_run(s, 3 * (n + 1), [&](int i) {
        const int j = i / 3 - 1;
        return ml_item_seg(j < 0 ? ml_append(ml_lit("dom-sep"), ml_zero_byte()) : item(j), i % 3);
    });
}

// add_to_transcript of a &[u8] (utils.rs:29-37): the message is u64le(len) ‖ bytes, absorbed as ONE AD operation in two
// parts, so a slice is four segments where an item is three
CG_HD MlSeg ml_slice_seg(MlLit label, const uint8_t* bytes, uint64_t len, int part) {
    if (part == 0) return MlSeg{ML_META_AD, false, label.len, nullptr, label, nullptr};
    if (part == 1) return MlSeg{ML_META_AD, true, 4, nullptr, ml_u32((uint32_t)(8 + len)), nullptr};
    if (part == 2) return MlSeg{ML_AD, false, 8, nullptr, ml_u64(len), nullptr};
    return MlSeg{ML_AD, true, (uint32_t)len, bytes, MlLit{0, 0, 0}, nullptr};
}

// ---- the shapes: every point a pointer to its 32 compressed bytes, every challenge written as 32 bytes (top byte 0) -------

// The range transcript up to c (com_q null) or up to rho; a null destination is drawn and dropped.
CG_HD void ml_range_challenges(uint8_t* st, const uint8_t* com_f, const uint8_t* com_g, const uint8_t* com_q, uint8_t* c, uint8_t* rho) {
    if (c) c[ML_CHALLENGE] = 0;
    if (rho) rho[ML_CHALLENGE] = 0;
    ml_transcript(st, com_q ? 5 : 3, [&](int j) {
        switch (j) {
            case 0: return ml_append(ml_lit("com_f"), com_f, 32);
            case 1: return ml_append(ml_lit("com_g"), com_g, 32);
            case 2: return ml_challenge(c);
            case 3: return ml_append(ml_lit("com_q"), com_q, 32);
            default: return ml_challenge(rho);
        }
    });
}

// The DLEQ of a range proof (rangeproof.rs:218-245, 416-423): context None; statement 0 the slot's two bases, k_0 and
// ped_com; statement 1 com_f_basis (4), k_1 and com_f.  slot_bases: 2 x 32 bytes, cf_basis: 4 x 32, k: k_0 ‖ k_1.
CG_HD void ml_range_dleq_challenge(uint8_t* st, const uint8_t* slot_bases, const uint8_t* cf_basis, const uint8_t* k,
                                   const uint8_t* ped_com, const uint8_t* com_f, uint8_t* c) {
    c[ML_CHALLENGE] = 0;
    ml_transcript(st, 14, [&](int j) {
        switch (j) {
            case 0: return ml_append(ml_lit("context string"), ml_u64(0));
            case 1: return ml_append(ml_lit("num_bases"), ml_u64(2));
            case 2: case 3: return ml_append(ml_lit("base"), slot_bases + 32 * (j - 2), 32);
            case 4: return ml_append(ml_lit("k"), k, 32);
            case 5: return ml_append(ml_lit("y"), ped_com, 32);
            case 6: return ml_append(ml_lit("num_bases"), ml_u64(4));
            case 7: case 8: case 9: case 10: return ml_append(ml_lit("base"), cf_basis + 32 * (j - 7), 32);
            case 11: return ml_append(ml_lit("k"), k + 32, 32);
            case 12: return ml_append(ml_lit("y"), com_f, 32);
            default: return ml_challenge(c);
        }
    });
}

// DLogPoK's transcript for any shape (dlog.rs:56-58, 77-99; :130-132, 147-169), one text for host and device: the context
// as a slice (null with length 0 is `None`), then per statement i its n_bases(i) bases - taken in order from `bases` -
// under b"num_bases" and b"base", k + 32 i under b"k" and y + 32 i under b"y", then the challenge.  Which statement an
// item belongs to is found by walking the counts: a showing has a handful of statements.  c: 32 bytes.
template <class CountFn>
CG_HD void ml_dlog_shape_challenge(uint8_t* st, const uint8_t* context, uint64_t context_len, uint32_t n_statements, CountFn n_bases,
                                   const uint8_t* bases, const uint8_t* k, const uint8_t* y, uint8_t* c) {
    c[ML_CHALLENGE] = 0;
    uint32_t n_items = 1;
    for (uint32_t i = 0; i < n_statements; ++i) n_items += n_bases(i) + 3;
    Strobe s = ml_strobe(st);
    ml_run(s, 7 + 3 * (int)n_items, [&](int seg) {
        if (seg < 3) return ml_item_seg(ml_append(ml_lit("dom-sep"), ml_zero_byte()), seg);
        if (seg < 7) return ml_slice_seg(ml_lit("context string"), context, context_len, seg - 3);
        const int part = (seg - 7) % 3;
        uint32_t j = (uint32_t)(seg - 7) / 3, i = 0, first = 0;
        if (j + 1 == n_items) return ml_item_seg(ml_challenge(c), part);
        while (j >= n_bases(i) + 3) {
            j -= n_bases(i) + 3;
            first += n_bases(i);
            ++i;
        }
        const uint32_t nb = n_bases(i);
        if (j == 0) return ml_item_seg(ml_append(ml_lit("num_bases"), ml_u64(nb)), part);
        if (j <= nb) return ml_item_seg(ml_append(ml_lit("base"), bases + 32 * (uint64_t)(first + j - 1), 32), part);
        if (j == nb + 1) return ml_item_seg(ml_append(ml_lit("k"), k + 32 * (uint64_t)i, 32), part);
        return ml_item_seg(ml_append(ml_lit("y"), y + 32 * (uint64_t)i, 32), part);
    });
}

// ark-serialize's compressed form of an uncompressed G1 point, by arithmetic on its 16 words alone: x with the
// infinity flag carried over, or with YIsNegative where y > q - y.  Nothing is checked; a point that a checked
// deserialisation refuses still gives 8 words.
CG_HD void ml_compress_g1(const uint32_t* w, uint32_t* out) {
    const uint32_t flag = w[15] >> 30;
    uint32_t y[8], ny[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) y[i] = w[8 + i];
    y[7] &= 0x3fffffffu;
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t d = (uint64_t)FqP::N[i] - y[i] - borrow;
        ny[i] = (uint32_t)d;
        borrow = (uint32_t)(d >> 63);
    }
    bool nonzero = false, neg = false, decided = false;                     // neg: q - y < y
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        nonzero = nonzero || y[i] != 0;
        if (!decided && ny[i] != y[i]) {
            neg = ny[i] < y[i];
            decided = true;
        }
    }
    const bool inf = flag & 1u;
    for (int i = 0; i < 8; ++i) out[i] = inf ? 0u : w[i];
    out[7] |= inf ? 0x40000000u : (neg && nonzero) ? 0x80000000u : 0u;
}

// ---- the host's general transcript: any label, any message, any number of bytes drawn (host functions) --------------------
struct MerlinTranscript {
    alignas(8) uint8_t st[ML_STATE];
    Strobe s;
    MerlinTranscript(const uint8_t* label, uint32_t len) : s(ml_strobe(st)) { append_message((const uint8_t*)"dom-sep", 7, label, len); }
    MerlinTranscript(const MerlinTranscript&) = delete;
    MerlinTranscript& operator=(const MerlinTranscript&) = delete;
    void op(const uint8_t* label, uint32_t label_len, uint8_t flags, const uint8_t* msg, uint32_t len, uint8_t* dst) {
        const MlSeg g[3] = {{ML_META_AD, false, label_len, label, MlLit{0, 0, 0}, nullptr},
                            {ML_META_AD, true, 4, nullptr, ml_u32(len), nullptr},
                            {flags, false, len, msg, MlLit{0, 0, 0}, dst}};
        ml_run(s, 3, [&](int i) { return g[i]; });
    }
    void append_message(const uint8_t* label, uint32_t label_len, const uint8_t* msg, uint32_t len) { op(label, label_len, ML_AD, msg, len, nullptr); }
    void challenge_bytes(const uint8_t* label, uint32_t label_len, uint8_t* out, uint32_t n) { op(label, label_len, ML_PRF, nullptr, n, out); }
    void append_slice(MlLit label, const uint8_t* bytes, uint64_t len) {
        ml_run(s, 4, [&](int i) { return ml_slice_seg(label, bytes, len, i); });
    }
    void append(const MlItem& it) {
        ml_run(s, 3, [&](int i) { return ml_item_seg(it, i); });
    }
};

// DLogPoK's transcript in general (dlog.rs:56-58, 77-99): statement i has n_bases[i] bases, taken in order from `bases`,
// then k + 32 i and y(i); every point 32 compressed bytes.  c: 32 bytes.
template <class YFn>
inline void ml_dlog_challenge(const uint8_t* context, uint64_t context_len, uint32_t n_statements, const uint32_t* n_bases,
                              const uint8_t* bases, const uint8_t* k, YFn y, uint8_t* c) {
    const uint8_t zero = 0;
    MerlinTranscript t(&zero, 1);
    t.append_slice(ml_lit("context string"), context, context_len);
    for (uint32_t i = 0; i < n_statements; ++i) {
        t.append(ml_append(ml_lit("num_bases"), ml_u64(n_bases[i])));
        for (uint32_t j = 0; j < n_bases[i]; ++j, bases += 32) t.append(ml_append(ml_lit("base"), bases, 32));
        t.append(ml_append(ml_lit("k"), k + 32 * (uint64_t)i, 32));
        t.append(ml_append(ml_lit("y"), y(i), 32));
    }
    c[ML_CHALLENGE] = 0;
    t.append(ml_challenge(c));
}

}  // namespace cg
