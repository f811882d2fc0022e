// The link between the two halves of a showing (creds/src/lib.rs:645-646, :847-848, :868-876 on the verifying side,
// :370-372, :468-470, :505-507 on the creating side): a range proof does not speak about a committed input of the showing
// but about that input shifted by a public value t (cur_time, or days_to_be_age(age) for an mDL attribute),
//   ped_com = committed - t·gamma_abc_g1[pos]        and, for whoever holds the opening,   m' = m - t mod r.
// Written once for host and device, next to the fixed-base walk it takes (fixed_base.hpp); tests/cpp/test_show_link.cpp
// runs it under plain g++.
#pragma once
#include "fixed_base.hpp"

namespace cg {

// a canonical scalar: 8 little-endian words below r
CG_HD bool link_below_r(const uint32_t a[8]) {
    for (int i = 7; i >= 0; --i) {
        if (a[i] < FrP::N[i]) return true;
        if (a[i] > FrP::N[i]) return false;
    }
    return false;
}

// committed - t·base from the 8-bit table of that base (a key's table of gamma_abc_g1[i+1]); t is any 256-bit integer.
// The last step is the general addition: a chosen input makes committed == t·base, where the result is O - a legal
// ped_com -, or committed == -t·base, which is a doubling; committed itself may be O.
template <class F>
CG_HD XYZZ<F> shift_commitment(const Affine<F>* tab_of_input, const Affine<F>& committed, const uint32_t t[8]) {
    XYZZ<F> acc = neg(fixed_base_mul(tab_of_input, t));
    add(acc, XYZZ<F>::from_affine(committed));
    return acc;
}

// m - t mod r for canonical m and t (m < t wraps), canonical
CG_HD void shift_opening(const uint32_t m[8], const uint32_t t[8], uint32_t out[8]) {
    Fr a, b;
    for (int i = 0; i < 8; ++i) {
        a.l[i] = m[i];
        b.l[i] = t[i];
    }
    const Fr d = sub(a, b);
    for (int i = 0; i < 8; ++i) out[i] = d.l[i];
}

}  // namespace cg
