// The two pieces of creating a whole showing (creds/src/lib.rs:364-373, :468-471, :505-509) that the host and the device
// must agree on word for word:
//   - one row of `DLogPoK::prove`'s responses (creds/src/dlog.rs:101-109), s = nonce - c·secret mod r, from canonical limbs;
//   - where the Pedersen opening of a range link lies in a showing's own data: the range proof of link j speaks about the
//     committed input `pos` of the showing, whose opening is `committed_input_openings[ci]` of groth16rand.rs:135-139,
//     (m, r) = (inputs[pos], r_ci), and r_ci is drawn into `rand` behind r1 and r2 (include/crescent_gpu.h,
//     cg_show_commit_batch: r1, r2, the r_i, z, the nonces).
// Written once for host and device, as show_link.hpp and rangepoly.hpp are: dlog_respond (key_handle.hpp, the host's
// responses) and k_mk_respond (verify.hip) take the same row; tests/cpp/test_show_make.cpp runs it under plain g++.
#pragma once
#include "field.hpp"

namespace cg {

// c in Montgomery form, once per showing: c·R times a canonical x is c·x, canonical
CG_HD Fr mk_challenge_mont(const uint32_t c[8]) {
    Fr a;
    for (int i = 0; i < 8; ++i) a.l[i] = c[i];
    return to_mont(a);
}

// s = nonce - c·secret mod r: secret and nonce canonical (below r), c as mk_challenge_mont gives it; s canonical
CG_HD void mk_response_row(const Fr& c_mont, const uint32_t secret[8], const uint32_t nonce[8], uint32_t s[8]) {
    Fr x, k;
    for (int i = 0; i < 8; ++i) {
        x.l[i] = secret[i];
        k.l[i] = nonce[i];
    }
    const Fr d = sub(k, mul(c_mont, x));
    for (int i = 0; i < 8; ++i) s[i] = d.l[i];
}

// The opening of a link in showing p, as scalar indices (8 words, 32 bytes each): m in the call's `inputs` (n_io per
// showing), r in its `rand` (n_rand per showing).  pos is the linked input's index into io_types, ci its rank among the
// committed inputs.
struct MkOpeningAt {
    uint64_t m, r;
};
CG_HD MkOpeningAt mk_link_opening(uint64_t p, uint32_t n_io, uint32_t n_rand, uint32_t pos, uint32_t ci) {
    return MkOpeningAt{p * n_io + pos, p * n_rand + 2 + ci};
}

}  // namespace cg
