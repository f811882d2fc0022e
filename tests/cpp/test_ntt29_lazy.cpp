// Host-side check of the transforms' lazy 29-bit-limb steps (csrc/field29.hpp weak_reduce, bfly, and the op order of
// csrc/wmap29.hip k_ntt29_pass) at the values random data never reaches: exact multiples of N, the largest representatives
// the packed form holds, tiles of equal values, outputs that are zero everywhere but one.  The replay below repeats the
// kernel's op order (as tools/bounds29.py repeats curve29.hpp's); the arithmetic it calls is the product's.  Compared
// element by element with a plain radix-2 transform in the saturated 8x32 field (csrc/field.hpp).  Plain g++; exits
// non-zero on the first mismatch.  Also asserts the bounds tools/bounds29.py check_ntt_pass proves.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../crescent-credentials_amd/csrc/field29.hpp"

using namespace cg;

#define CHECK(c, ...) do { if (!(c)) { printf("FAIL line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static uint64_t rng_s = 0x243f6a8885a308d3ull;
static uint64_t rnd() { rng_s ^= rng_s << 13; rng_s ^= rng_s >> 7; rng_s ^= rng_s << 17; return rng_s; }

// ---- a small big integer (320 bits) for the checks that must not go through the arithmetic under test ------------------------
struct Big {
    uint32_t w[10];
    static Big zero() { Big b; memset(b.w, 0, sizeof(b.w)); return b; }
    static Big from_limbs29(const uint32_t l[9]) {          // Σ l[i]·2^(29 i), limbs of any size
        Big b = zero();
        for (int i = 0; i < 9; ++i) {
            const int bit = 29 * i, wi = bit >> 5, sh = bit & 31;
            uint64_t v = (uint64_t)l[i] << sh, c = 0;
            for (int k = wi; k < 10; ++k) {
                uint64_t t = (uint64_t)b.w[k] + (uint32_t)v + c;
                b.w[k] = (uint32_t)t; c = t >> 32; v >>= 32;
                if (!v && !c) break;
            }
        }
        return b;
    }
    static Big modulus() { Big b = zero(); for (int i = 0; i < 8; ++i) b.w[i] = FrP::N[i]; return b; }
    int cmp(const Big& o) const {
        for (int i = 9; i >= 0; --i) if (w[i] != o.w[i]) return w[i] < o.w[i] ? -1 : 1;
        return 0;
    }
    Big shl(int s) const {                                    // s < 32
        Big r = zero();
        for (int i = 0; i < 10; ++i) {
            r.w[i] = w[i] << s;
            if (s && i) r.w[i] |= w[i - 1] >> (32 - s);
        }
        return r;
    }
    Big minus(const Big& o) const {
        Big r; uint64_t br = 0;
        for (int i = 0; i < 10; ++i) { uint64_t t = (uint64_t)w[i] - o.w[i] - br; r.w[i] = (uint32_t)t; br = (t >> 32) & 1u; }
        return r;
    }
    Big plus(const Big& o) const {
        Big r; uint64_t c = 0;
        for (int i = 0; i < 10; ++i) { uint64_t t = (uint64_t)w[i] + o.w[i] + c; r.w[i] = (uint32_t)t; c = t >> 32; }
        return r;
    }
    Big mod_n() const {                                       // value < 2^270
        Big r = *this; const Big n = modulus();
        for (int s = 16; s >= 0; --s) { Big t = n.shl(s); if (r.cmp(t) >= 0) r = r.minus(t); }
        return r;
    }
    Fr29 to_limbs29() const {                                 // value < 2^261 + a little: limb 8 takes the rest
        Fr29 r;
        for (int i = 0; i < 9; ++i) {
            const int bit = 29 * i, wi = bit >> 5, sh = bit & 31;
            uint64_t v = w[wi] | ((uint64_t)w[wi + 1] << 32);
            r.l[i] = (uint32_t)(v >> sh) & (i < 8 ? M29 : 0xffffffffu);
        }
        return r;
    }
};
static Big big_kn(int k) { Big r = Big::zero(); const Big n = Big::modulus(); for (int i = 0; i < k; ++i) r = r.plus(n); return r; }
static Big value_of(const Fr29& a) { return Big::from_limbs29(a.l); }
static bool normalised(const Fr29& a) { for (int i = 0; i < 8; ++i) if (a.l[i] > M29) return false; return true; }
static bool same_limbs(const Fr29& a, const Fr29& b) { return memcmp(a.l, b.l, sizeof(a.l)) == 0; }

// ---- 3a: weak_reduce -----------------------------------------------------------------------------------------------------------
static double weak_max = 0.0;
static void check_weak_reduce(const Fr29& v, const char* what) {
    CHECK(normalised(v) && v.l[8] < (1u << 29), "%s: the input is not a normalised value below 2^261", what);
    const Fr29 r = weak_reduce(v);
    CHECK(normalised(r), "%s: result not normalised", what);
    const Big rv = value_of(r), want = value_of(v).mod_n();
    CHECK(rv.cmp(big_kn(3)) < 0, "%s: result not below 3N (top limb %u)", what, r.l[8]);
    CHECK(rv.mod_n().cmp(want) == 0, "%s: result not congruent to the input", what);
    CHECK(to_canonical_bytes(r) == to_canonical_bytes(want.to_limbs29()), "%s: canonical bytes differ", what);
    uint32_t w[8];
    pack29(r, w);
    CHECK(same_limbs(unpack29<Fr29P>(w), r), "%s: the packed form does not hold the result", what);
    weak_max = std::max(weak_max, (double)(r.l[8] + 1) / 3171406.0);
}
static void test_weak_reduce() {
    const Big n = Big::modulus();
    Big one = Big::zero(); one.w[0] = 1;
    check_weak_reduce(Big::zero().to_limbs29(), "0");
    check_weak_reduce(n.minus(one).to_limbs29(), "N-1");
    check_weak_reduce(n.plus(one).to_limbs29(), "N+1");
    for (int k = 0; k <= 60; ++k) {
        char nm[16]; snprintf(nm, sizeof nm, "%d*N", k);
        check_weak_reduce(big_kn(k).to_limbs29(), nm);
        if (k) check_weak_reduce(big_kn(k).minus(one).to_limbs29(), "k*N-1");
    }
    check_weak_reduce(big_kn(169).to_limbs29(), "169*N");              // the largest multiple below 2^261
    Fr29 t;
    for (int i = 0; i < 9; ++i) t.l[i] = M29;
    check_weak_reduce(t, "2^261-1");
    t.l[8] = (1u << 24) - 1;
    check_weak_reduce(t, "2^256-1");
    for (int it = 0; it < 100000; ++it) {
        for (int i = 0; i < 9; ++i) t.l[i] = (uint32_t)rnd() & M29;
        if ((it & 3) == 1) t.l[8] >>= (rnd() % 29);                    // small values too
        check_weak_reduce(t, "random");
    }
    printf("weak_reduce ok: every result below %.4f N (contract 3 N)\n", weak_max);
    CHECK(weak_max < 3.0, "weak_reduce above its contract");
}

// ---- 3b: one tile of k_ntt29_pass on the host -----------------------------------------------------------------------------------
static Fr fr_small(uint32_t v) { Fr a = Fr::zero(); a.l[0] = v; return to_mont(a); }
static Fr fr_pow(const Fr& a, uint64_t e) { uint32_t l[8] = {(uint32_t)e, (uint32_t)(e >> 32), 0, 0, 0, 0, 0, 0}; return pow_limbs(a, l); }
static Fr root_of_unity(int logn) {            // 5^((r-1)/2^28) squared 28 - logn times (the oracle's root_of_unity)
    uint32_t e[8];
    for (int i = 0; i < 8; ++i) e[i] = FrP::N[i];
    e[0] -= 1u;
    for (int i = 0; i < 8; ++i) e[i] = (e[i] >> 28) | (i < 7 ? e[i + 1] << 4 : 0u);
    Fr w = pow_limbs(fr_small(5), e);
    for (int i = logn; i < 28; ++i) w = sqr(w);
    return w;
}
static Fr rand_fr() {
    Fr a;
    for (;;) {
        for (int i = 0; i < 8; ++i) a.l[i] = (uint32_t)rnd();
        a.l[7] &= 0x3fffffffu;
        for (int i = 7; i >= 0; --i) { if (a.l[i] < FrP::N[i]) return a; if (a.l[i] > FrP::N[i]) break; }
    }
}
static uint32_t brev(uint32_t x, int bits) { uint32_t r = 0; for (int i = 0; i < bits; ++i) r |= ((x >> i) & 1u) << (bits - 1 - i); return r; }

// what the kernel reads from global memory: eight words, unpacked
static Fr29 through_packed(const Fr29& a) { uint32_t w[8]; pack29(a, w); return unpack29<Fr29P>(w); }
// the largest representative of a canonical value that the packed form holds (value + k·N < 2^256)
static Fr29 lifted(Fr29 x) {
    const Fr29 n = Fr29::from_limbs(Fr29P::N);
    for (;;) { Fr29 y = normalize(add(x, n)); if (y.l[8] >= (1u << 24)) return x; x = y; }
}
// a weak_reduce output: the value plus a random multiple of N below 2^261, reduced as a pass's STORE 0 reduces it
static Fr29 weakly_reduced(Fr29 x) {
    const Fr29 n = Fr29::from_limbs(Fr29P::N);
    for (int k = (int)(rnd() % 160); k > 0; --k) x = normalize(add(x, n));
    return weak_reduce(x);
}

// the elements one column of a pass works on: 2^S values whose global indices differ in bits [gbit_lo, gbit_lo + S)
struct Column {
    int logn, q0, S, gbit_lo;
    uint32_t rest;                                   // the other bits of the global index, in place
    uint32_t gi(uint32_t g) const { return rest | (g << gbit_lo); }
};
struct Seen {
    uint32_t limb = 0; double value = 0.0;           // before a normalize: the largest limb, the largest value / N
    void see(const Fr29& x) {
        for (int i = 0; i < 8; ++i) limb = std::max(limb, x.l[i]);
        value = std::max(value, (double)(normalize(x).l[8] + 1) / 3171406.0);   // N / 2^232 = 3171406.5
    }
};

// stages q0 .. q0 + S - 1 as k_ntt29_pass takes them: radix-4 groups in registers, one normalize per element and pair, the
// product-free first group of a transform, an odd last stage radix-2
static void replay_pass(std::vector<Fr29>& x, const Column& c, const std::vector<Fr29>& tw, Seen& seen) {
    auto put = [&](Fr29& dst, const Fr29& v) { seen.see(v); dst = normalize(v); };
    int j = 0;
    for (; j + 1 < c.S; j += 2) {
        const int q = c.q0 + j, sh1 = c.logn - 1 - q, sh2 = c.logn - 2 - q;
        const uint32_t lmask = (1u << j) - 1u;
        for (uint32_t b = 0; b < (1u << c.S) >> 2; ++b) {
            const uint32_t g00 = ((b & ~lmask) << 2) | (b & lmask), g01 = g00 | (1u << j), g10 = g00 | (2u << j), g11 = g00 | (3u << j);
            const uint32_t k = c.gi(g00) & ((1u << q) - 1u);
            Fr29 x0 = x[g00], x1 = x[g01], x2 = x[g10], x3 = x[g11];
            if (q == 0) {
                Fr29 t = x1;
                x1 = sub<7, 1>(x0, t);
                x0 = add(x0, t);
                t = x3;
                x3 = sub<7, 1>(x2, t);
                x2 = add(x2, t);
                t = x2;
                x2 = sub<12, 2>(x0, t);
                x0 = add(x0, t);
                bfly(x1, x3, tw[(size_t)1 << sh2]);
            } else {
                const Fr29 w1 = tw[(size_t)k << sh1], w2a = tw[(size_t)k << sh2], w2b = tw[(size_t)(k + (1u << q)) << sh2];
                bfly(x0, x1, w1);
                bfly(x2, x3, w1);
                bfly(x0, x2, w2a);
                bfly(x1, x3, w2b);
            }
            put(x[g00], x0); put(x[g01], x1); put(x[g10], x2); put(x[g11], x3);
        }
    }
    if (j < c.S) {
        const int q = c.q0 + j;
        const uint32_t lmask = (1u << j) - 1u;
        for (uint32_t b = 0; b < (1u << c.S) >> 1; ++b) {
            const uint32_t g0 = ((b & ~lmask) << 1) | (b & lmask), g1 = g0 | (1u << j);
            const uint32_t k = c.gi(g0) & ((1u << q) - 1u);
            Fr29 u = x[g0], v = x[g1];
            bfly(u, v, tw[(size_t)k << (c.logn - 1 - q)]);
            put(x[g0], u); put(x[g1], v);
        }
    }
}
// the same stages as plain radix-2 butterflies in the saturated field
static void plain_stages(std::vector<Fr>& x, const Column& c, const std::vector<Fr>& tw) {
    for (int j = 0; j < c.S; ++j) {
        const int q = c.q0 + j;
        for (uint32_t g = 0; g < (1u << c.S); ++g) {
            if (g & (1u << j)) continue;
            const uint32_t k = c.gi(g) & ((1u << q) - 1u);
            const Fr t = mul(x[g | (1u << j)], tw[(size_t)k << (c.logn - 1 - q)]);
            x[g | (1u << j)] = sub(x[g], t);
            x[g] = add(x[g], t);
        }
    }
}

struct Tables {
    int logn;
    std::vector<Fr> tw;            // ω^i, i < n/2, Montgomery(2^256)
    std::vector<Fr29> tw29;        // the same in R' form, canonical (k_to_limbs12)
    Fr omega;
    explicit Tables(int logn_) : logn(logn_) {
        omega = root_of_unity(logn);
        const size_t half = logn ? (size_t)1 << (logn - 1) : 1;
        tw.resize(half); tw29.resize(half);
        Fr w = Fr::one();
        for (size_t i = 0; i < half; ++i) { tw[i] = w; tw29[i] = from_mont256<Fr29P>(w); w = mul(w, omega); }
    }
};

// every STORE form of the pass on the replayed values against the plain ones
static void check_stores(const std::vector<Fr29>& x, const std::vector<Fr>& want, const char* what) {
    const Fr c_m = rand_fr();                                    // STORE 2's constant (plain 1/n in the product)
    const Fr c_plain = from_mont(c_m);
    for (size_t i = 0; i < x.size(); ++i) {
        CHECK(normalised(x[i]), "%s: element %zu not normalised after the last stage", what, i);
        // STORE 0
        const Fr29 y0 = weak_reduce(x[i]);
        CHECK(normalised(y0) && value_of(y0).cmp(big_kn(3)) < 0, "%s: STORE 0 element %zu not below 3N", what, i);
        CHECK(same_limbs(through_packed(y0), y0), "%s: STORE 0 element %zu does not fit the packed form", what, i);
        CHECK(to_canonical_bytes(y0) == from_mont(want[i]), "%s: STORE 0 element %zu differs", what, i);
        // STORE 1: a canonical R'-form factor per element
        const Fr s_m = (i % 7 == 3) ? Fr::zero() : rand_fr();
        const Fr29 y1 = cond_sub_n(mul(x[i], through_packed(from_mont256<Fr29P>(s_m))));
        CHECK(same_limbs(y1, from_mont256<Fr29P>(mul(want[i], s_m))), "%s: STORE 1 element %zu differs or is not canonical", what, i);
        // STORE 2: one plain constant; STORE 3: a plain canonical factor per element, as the first operand
        uint32_t w[8];
        pack29(cond_sub_n(mul(x[i], unpack29<Fr29P>(c_plain.l))), w);
        Fr e = from_mont(mul(want[i], c_m));
        CHECK(memcmp(w, e.l, 32) == 0, "%s: STORE 2 element %zu differs", what, i);
        const Fr b_m = rand_fr();
        pack29(cond_sub_n(mul(unpack29<Fr29P>(from_mont(b_m).l), x[i])), w);
        e = from_mont(mul(want[i], b_m));
        CHECK(memcmp(w, e.l, 32) == 0, "%s: STORE 3 element %zu differs", what, i);
    }
}

static Seen seen_first[2], seen_strided[2];      // [0]: the 10-stage / 6-stage shapes, [1]: the 11-stage / 10-stage ones

// a whole transform of 2^logn points as ONE first pass: input in natural order (Montgomery form), read bit-reversed
// lift: 0 = canonical inputs, 1 = every input lifted, 2 = only the subtrahends of the first group's second stage (its third and
// fourth element), the minuends zero: the edge sub<12,2> is sized for
static void run_first_pass(const Tables& T, const std::vector<Fr>& in, int lift, Seen& seen, const char* what, long only_nonzero = -2) {
    const int logn = T.logn;
    const uint32_t n = 1u << logn;
    const Column c{logn, 0, logn, 0, 0u};
    std::vector<Fr29> x(n);
    std::vector<Fr> ref(n);
    for (uint32_t e = 0; e < n; ++e) {
        const Fr v = (lift == 2 && !(e & 2u)) ? Fr::zero() : in[brev(e, logn)];
        Fr29 p = from_mont256<Fr29P>(v);
        x[e] = through_packed((lift == 1 || (lift == 2 && (e & 2u))) ? lifted(p) : p);
        ref[e] = v;
    }
    replay_pass(x, c, T.tw29, seen);
    plain_stages(ref, c, T.tw);
    if (only_nonzero != -2)                          // the closed form: zero everywhere but one index (or everywhere)
        for (uint32_t i = 0; i < n; ++i) CHECK(ref[i].is_zero() == ((long)i != only_nonzero), "%s: closed form broken at %u", what, i);
    check_stores(x, ref, what);
}
static void test_first_pass(int logn, Seen& seen) {
    const Tables T(logn);
    const uint32_t n = 1u << logn;
    std::vector<Fr> in(n);
    char what[96];
    for (int lift = 0; lift < 2; ++lift) {
        for (auto& v : in) v = rand_fr();
        in[1] = Fr::zero(); in[2] = fr_small(1);
        snprintf(what, sizeof what, "2^%d random%s", logn, lift ? " lifted" : "");
        run_first_pass(T, in, lift, seen, what);
        // all equal: 1, r - 1, (r - 1)/2: every output but the first is zero
        const Fr one = fr_small(1), r1 = neg(one), half = mul(r1, inv(fr_small(2)));
        const Fr cs[3] = {one, r1, half};
        for (int ci = 0; ci < 3; ++ci) {
            for (auto& v : in) v = cs[ci];
            snprintf(what, sizeof what, "2^%d all equal (c%d)%s", logn, ci, lift ? " lifted" : "");
            run_first_pass(T, in, lift, seen, what, 0);
            // geometric: x_i = c·ω^(-k0·i) -> n·c at k0, zero elsewhere
            const uint32_t k0s[4] = {1u, n / 2, n - 1, (n / 3) | 1u};
            for (uint32_t k0 : k0s) {
                const Fr step = fr_pow(T.omega, n - k0);
                Fr v = cs[ci];
                for (uint32_t i = 0; i < n; ++i) { in[i] = v; v = mul(v, step); }
                snprintf(what, sizeof what, "2^%d geometric k0=%u (c%d)%s", logn, k0, ci, lift ? " lifted" : "");
                run_first_pass(T, in, lift, seen, what, (long)k0);
            }
        }
        for (auto& v : in) v = Fr::zero();
        snprintf(what, sizeof what, "2^%d all zero%s", logn, lift ? " lifted" : "");
        run_first_pass(T, in, lift, seen, what, -1);
    }
    for (auto& v : in) v = rand_fr();
    snprintf(what, sizeof what, "2^%d zero minuends, lifted subtrahends", logn);
    run_first_pass(T, in, 2, seen, what);
    printf("first pass of %d stages ok: values before normalize up to %.2f N, limbs up to %.2f * 2^29\n", logn, seen.value,
           (double)seen.limb / (double)(1u << 29));
}

// one column of a strided pass of S stages in a transform of 2^logn points, entered with weak_reduce outputs
static void test_strided(int logn, int ts, int S, Seen& seen) {
    const Tables T(logn);
    const int gbit_lo = ts, n_cols = 6;
    char what[96];
    for (int col = 0; col < n_cols; ++col) {
        // the bits below gbit_lo and above gbit_lo + S: none, all, random
        uint32_t rest = col == 0 ? 0u : col == 1 ? 0xffffffffu : (uint32_t)rnd();
        rest &= ((1u << logn) - 1u) & ~(((1u << S) - 1u) << gbit_lo);
        const Column c{logn, ts, S, gbit_lo, rest};
        for (int fam = 0; fam < 6; ++fam) {
            std::vector<Fr29> x((size_t)1 << S);
            std::vector<Fr> ref(x.size());
            const Fr one = fr_small(1), r1 = neg(one), half = mul(r1, inv(fr_small(2)));
            for (size_t g = 0; g < x.size(); ++g) {
                Fr v = fam == 0 ? rand_fr() : fam == 1 ? one : fam == 2 ? r1 : fam == 3 ? half : fam == 4 ? Fr::zero()
                                                                                               : ((g & 1) ? Fr::zero() : rand_fr());
                ref[g] = v;
                x[g] = through_packed(weakly_reduced(from_mont256<Fr29P>(v)));
            }
            snprintf(what, sizeof what, "2^%d strided %d stages, column %d, family %d", logn, S, col, fam);
            replay_pass(x, c, T.tw29, seen);
            plain_stages(ref, c, T.tw);
            check_stores(x, ref, what);
        }
    }
    printf("strided pass of %d stages (2^%d) ok: values before normalize up to %.2f N, limbs up to %.2f * 2^29\n", S, logn, seen.value,
           (double)seen.limb / (double)(1u << 29));
}

int main() {
    test_weak_reduce();
    test_first_pass(10, seen_first[0]);
    test_first_pass(11, seen_first[1]);
    test_strided(16, 10, 6, seen_strided[0]);
    test_strided(21, 11, 10, seen_strided[1]);
    // the bounds tools/bounds29.py check_ntt_pass prints for these four shapes, and its limb bound
    const double proven[4] = {46.58, 49.58, 21.00, 33.00};
    const Seen* s[4] = {&seen_first[0], &seen_first[1], &seen_strided[0], &seen_strided[1]};
    for (int i = 0; i < 4; ++i) {
        CHECK(s[i]->value < proven[i], "shape %d: value %.2f N above the proven bound %.2f N", i, s[i]->value, proven[i]);
        CHECK((uint64_t)s[i]->limb <= 5ull << 29, "shape %d: limb %u above 5 * 2^29", i, s[i]->limb);
    }
    printf("observed / proven value bounds: %.2f / %.2f, %.2f / %.2f, %.2f / %.2f, %.2f / %.2f N\n", s[0]->value, proven[0], s[1]->value,
           proven[1], s[2]->value, proven[2], s[3]->value, proven[3]);
    printf("ALL OK\n");
    return 0;
}
