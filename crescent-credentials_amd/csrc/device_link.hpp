// The BN254 half of `DeviceProof::verify` (creds/src/device.rs:168-213): what host and device must agree on, written once
// for both, one lane per proof, as rangeverify.hpp is; tests/cpp/test_device_link.cpp runs it under plain g++.
//   - the TEXT FORMS the reference feeds to SHA-256 (device.rs:185-194: `to_string()` of arkworks 0.4 values), one rule per
//     function: dl_dec (a field element), dl_point_open / dl_point_sep / dl_point_close / dl_point_infinity (a G1 point).
//     UNVERIFIED in the sense of DESIGN.md §3: arkworks is not available to this project and the reference pins no such
//     string, so the three rules are restated from the 0.4 sources - `Display for Fp` is
//     `into_bigint().to_string().trim_start_matches('0')`, so ZERO IS THE EMPTY STRING; `Display for Affine` is "infinity" or
//     "(x, y)"; `Projective` prints its affine form - until an arkworks-made DeviceProof meets this code.  A correction is one
//     line here and one in tests/device_link_vectors.py.
//   - the message and the challenge: b"computing challenge for linking proof" ‖ dec(pi0.c) ‖ text(com0) ‖ text(proof.com1) ‖
//     text(comz) ‖ h_Q through sha256.hpp; e1 = the little-endian integer of digest[0..16), e2 of digest[16..32), both below
//     2^128 < r
//   - the scalar stage: the range checks, pi0's eq_pos comparison s[0][0] == s[1][0] (dlog.rs:155-164) and the merged scalars
//     of c1·lhs1 = c1·com0 + (c1 e1)·proof.com1 + (c1 e2)·comz - (c1 m)·g, so that every chain of a proof starts at once
//     (csrc/devicelink.hip has the terms).  Merging scalars does not change the group elements.
#pragma once
#include <string.h>

#include "sha256.hpp"
#include "show_link.hpp"

namespace cg {

// ---- the text forms ---------------------------------------------------------------------------------------------------
constexpr int DL_DIGITS = 81;              // nine chunks of nine digits: 10^81 > 2^256
constexpr int DL_DIGITS_ROOM = 84;         // what a caller sets aside for them
constexpr uint32_t DL_H_MAX = 64;          // bytes of h_Q at the most (compute_hQ returns the 32 of a P-256 field element)

// dec(v): the decimal digits of the 256-bit integer v[0..8) (top word and-ed with top_mask) with no leading zero, written
// RIGHT-ALIGNED into digits[0..DL_DIGITS); returns their number: the text is digits + DL_DIGITS - n.  Zero has no digit.
// Repeated division by 10^9, eight words at a time with constant indices; only the digit bytes are addressed at run time.
CG_HD uint32_t dl_dec(const uint32_t* v, uint32_t top_mask, uint8_t* digits) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = v[i];
    w[7] &= top_mask;
#pragma nounroll
    for (int it = 0; it < 9; ++it) {
        uint64_t rem = 0;
#pragma unroll
        for (int i = 7; i >= 0; --i) {
            const uint64_t cur = (rem << 32) | w[i];
            const uint64_t q = cur / 1000000000ull;
            rem = cur - q * 1000000000ull;
            w[i] = (uint32_t)q;
        }
        uint32_t chunk = (uint32_t)rem;
        uint8_t* d = digits + DL_DIGITS - 9 * (it + 1);
#pragma nounroll
        for (int j = 8; j >= 0; --j) {
            const uint32_t q = chunk / 10u;
            d[j] = (uint8_t)('0' + (chunk - 10u * q));
            chunk = q;
        }
    }
    uint32_t lead = 0;
    while (lead < (uint32_t)DL_DIGITS && digits[lead] == '0') ++lead;
    return (uint32_t)DL_DIGITS - lead;
}
// a G1 point: "infinity", or "(" dec(x) ", " dec(y) ")"
CG_HD constexpr MlLit dl_point_infinity() { return ml_lit("infinity"); }
CG_HD constexpr MlLit dl_point_open() { return ml_lit("("); }
CG_HD constexpr MlLit dl_point_sep() { return ml_lit(", "); }
CG_HD constexpr MlLit dl_point_close() { return ml_lit(")"); }

// ---- the message and the challenge --------------------------------------------------------------------------------------
// The digest of one proof's message.  c0: pi0.c, 8 words; com0, com1, comz: 16 words each as ark-serialize's uncompressed
// bytes stand (a point whose infinity flag is set is "infinity" whatever its coordinates hold); h_q: h_len bytes.
// blk: SHA_BLOCK bytes, 4-byte aligned; digits: DL_DIGITS_ROOM bytes; both named by the caller, LDS on the device.
// The message is walked in nine parts - the label, dec(pi0.c), six coordinates, h_Q - of up to three segments each, through
// ONE call site of sha_run: nothing of it is held beyond one coordinate's digits.
CG_HD void dl_challenge_digest(uint8_t* blk, uint8_t* digits, const uint32_t* c0, const uint32_t* com0, const uint32_t* com1,
                               const uint32_t* comz, const uint8_t* h_q, uint32_t h_len, uint8_t out[32]) {
    Sha256 s = sha_begin(blk);
#pragma nounroll
    for (int part = 0; part < 9; ++part) {
        ShaSeg a = sha_zeros(0), b = sha_zeros(0), c = sha_zeros(0);
        if (part == 0) {                                           // b"computing challenge for linking proof"
            a = sha_lit(ml_lit("computing challe"));
            b = sha_lit(ml_lit("nge for linking "));
            c = sha_lit(ml_lit("proof"));
        } else if (part == 8) {
            a = sha_bytes(h_q, h_len);
        } else if (part == 1) {
            const uint32_t n = dl_dec(c0, 0xffffffffu, digits);
            b = sha_bytes(digits + DL_DIGITS - n, n);
        } else {
            const uint32_t* pt = part < 4 ? com0 : part < 6 ? com1 : comz;
            const bool is_x = (part & 1) == 0, inf = (pt[15] >> 30) == 1u;
            if (inf) {
                if (is_x) a = sha_lit(dl_point_infinity());
            } else {
                const uint32_t n = dl_dec(is_x ? pt : pt + 8, is_x ? 0xffffffffu : 0x3fffffffu, digits);
                b = sha_bytes(digits + DL_DIGITS - n, n);
                if (is_x) {
                    a = sha_lit(dl_point_open());
                    c = sha_lit(dl_point_sep());
                } else {
                    c = sha_lit(dl_point_close());
                }
            }
        }
        sha_run(s, 3, part == 8, [&](int i) { return i == 0 ? a : i == 1 ? b : c; });
    }
    sha_digest(s, out);
}

// ---- the scalar stage ---------------------------------------------------------------------------------------------------
// the terms of the group stage, in the order csrc/devicelink.hip lays them out.  Fixed-base: g = gamma_abc_g1[pos0 + 1],
// g' = gamma_abc_g1[pos1 + 1], h = delta_g1
enum {
    DL_F_S00 = 0,      // pi0.s[0][0] g'
    DL_F_S01,          // pi0.s[0][1] h
    DL_F_S10,          // pi0.s[1][0] g
    DL_F_S11,          // pi0.s[1][1] h
    DL_F_T0,           // pi1.s[0][0] h
    DL_F_U0,           // pi1.s[1][0] g
    DL_F_U1,           // pi1.s[1][1] h
    DL_F_M,            // m g, subtracted (lhs1)
    DL_F_C1M,          // (c1 m) g, subtracted (c1 lhs1)
    DL_N_FIXED
};
enum {
    DL_V_C0_COM1O = 0, // pi0.c com1_orig
    DL_V_C0_COM1,      // pi0.c proof.com1
    DL_V_C1_COMZ,      // pi1.c comz
    DL_V_C1_COM0,      // pi1.c com0
    DL_V_C1E1_COM1,    // (c1 e1) proof.com1
    DL_V_C1E2_COMZ,    // (c1 e2) comz
    DL_V_E1_COM1,      // e1 proof.com1, 128 bits
    DL_V_E2_COMZ,      // e2 comz, 128 bits
    DL_N_VAR
};
// the merged scalars the stage writes; every other scalar is read where the caller put it
enum { DL_S_C1E1 = 0, DL_S_C1E2, DL_S_C1M, DL_N_SCALARS };
// the points that go out compressed: lhs1, then the two k of pi0 and the two of pi1
enum { DL_O_LHS1 = 0, DL_O_K00, DL_O_K01, DL_O_K10, DL_O_K11, DL_N_OUT };

enum : uint32_t { DL_MALFORMED = 1u, DL_EQ_POS = 2u };

struct DlIn {                  // canonical scalars as the caller passed them
    const uint32_t* m;
    const uint32_t* pi0_c;
    const uint32_t* pi0_s;     // 4 x 8 words: s[0][0], s[0][1], s[1][0], s[1][1]
    const uint32_t* pi1_c;
    const uint32_t* pi1_s;     // 3 x 8 words: s[0][0], s[1][0], s[1][1]
    const uint32_t* e;         // the digest: e1 (4 words) ‖ e2 (4 words)
};

CG_HD Fr dl_load(const uint32_t* w, int n_words) {
    Fr a = Fr::zero();
    for (int i = 0; i < n_words; ++i) a.l[i] = w[i];
    return a;
}

// Returns DL_MALFORMED, or the eq_pos bit; the merged scalars go to out[8 (t stride + l)], canonical, and only for a proof
// that is not malformed.  `stride` is the distance between two terms in scalars (1 on the host; the chunk size on the
// device, whose buffers are term-major).
CG_HD uint32_t dl_scalars(const DlIn& in, uint32_t* out, uint64_t stride) {
    bool ok = link_below_r(in.m) && link_below_r(in.pi0_c) && link_below_r(in.pi1_c);
    for (int j = 0; j < 4; ++j) ok = ok && link_below_r(in.pi0_s + 8 * j);
    for (int j = 0; j < 3; ++j) ok = ok && link_below_r(in.pi1_s + 8 * j);
    if (!ok) return DL_MALFORMED;
    bool eq = true;
    for (int l = 0; l < 8; ++l) eq = eq && in.pi0_s[l] == in.pi0_s[16 + l];
    const Fr c1 = to_mont(dl_load(in.pi1_c, 8));
    auto put = [&](int t, const Fr& x) {                           // c1 x, canonical
        const Fr v = from_mont(mul(c1, to_mont(x)));
        for (int l = 0; l < 8; ++l) out[8 * (uint64_t)t * stride + l] = v.l[l];
    };
    put(DL_S_C1E1, dl_load(in.e, 4));
    put(DL_S_C1E2, dl_load(in.e + 4, 4));
    put(DL_S_C1M, dl_load(in.m, 8));
    return eq ? DL_EQ_POS : 0u;
}

// ---- what the two transcripts absorb besides a proof's own points -------------------------------------------------------------
// The two contexts (2 x DL_CTX_LEN bytes), then the bases g', h, g, h compressed (4 x 32): pi0 absorbs all four, pi1 the last
// three.  base_bytes: gamma_abc_g1[1..] and then delta_g1 as the key's bytes hold them, 64 B each (n_io + 1 points).  Host only;
// the verifying and the creating call write the same bytes.
constexpr uint32_t DL_CTX_LEN = 42;
constexpr uint32_t DL_CONSTS_LEN = 2 * DL_CTX_LEN + 4 * 32;
inline void dl_link_consts(const uint8_t* base_bytes, uint64_t n_io, uint32_t pos0, uint32_t pos1, uint8_t consts[DL_CONSTS_LEN]) {
    memcpy(consts, "creating sigma proof pi0 for linking proof", DL_CTX_LEN);
    memcpy(consts + DL_CTX_LEN, "creating sigma proof pi1 for linking proof", DL_CTX_LEN);
    const uint64_t base_of[4] = {pos1, n_io, pos0, n_io};
    for (int i = 0; i < 4; ++i) {
        uint32_t w[16], c[8];
        memcpy(w, base_bytes + 64 * base_of[i], 64);
        ml_compress_g1(w, c);
        memcpy(consts + 2 * DL_CTX_LEN + 32 * i, c, 32);
    }
}

}  // namespace cg

#ifdef __HIPCC__
// ---- the internal entry of verify.hip, for csrc/devicelink.hip: what cg_device_link_verify_batch needs of a cg_pvk, whose
// type that file does not see.  The caller takes the lock for the whole call and works on the key's own stream.
#include <mutex>

#include "common.hpp"

namespace cg {
struct PvkLinkView {
    std::mutex* mu;
    int device;
    hipStream_t st;
    const G1Affine* tab;           // the key's fixed-base tables: table i is gamma_abc_g1[i + 1]'s, table n_io delta_g1's
    const uint8_t* base_bytes;     // the same points as the key's bytes hold them, 64 B each, in the same order
    uint64_t n_io;
    uint32_t n_com, ci0, ci1;      // committed inputs of the layout; the committed indices of pos0 and pos1
    // the per-call arrays of the device link: created by the first call, under the lock, and freed with the handle after its
    // streams have been waited for.  The verifying call (devicelink.hip), the creating call and the h_Q entries (both
    // devicelinkmake.hip) and the P-256 entries (p256tu.hip) have a slot each, so that calls of different kinds on one handle
    // do not evict each other.
    void** state;
    void (**state_free)(void*);
    void** make_state;
    void (**make_state_free)(void*);
    void** hq_state;
    void (**hq_state_free)(void*);
    void** p256_state;
    void (**p256_state_free)(void*);
};
// what needs no layout: everything but n_com, ci0 and ci1
void pvk_link_handle(cg_pvk* k, PvkLinkView& v);
// the whole view after the argument checks of the layout (verify.hip's io_layout) and of pos0 / pos1; CG_OK, or the failure
// already recorded.  No HIP call.
int pvk_link_view(cg_pvk* k, const uint8_t* io_types, uint64_t n_io, uint32_t pos0, uint32_t pos1, PvkLinkView& v);
}  // namespace cg
#endif
