"""Proving keys given by discrete logarithms, for the load-time key fold (csrc/ecntt.hip) on keys that hit its rare branches.

A key made from a random trapdoor has distinct, generic h-query points, and then the butterflies of the two inverse DFTs over
G1 (k_ec_stage), the per-wire sums of the C terms (k_ec_terms, k_accum_xyzz under sum_xyzz_by_key) and the fold itself
(k_ec_fold_l) only ever add unrelated finite points.  Here every key point is d·G for a chosen integer d mod r (0: the
identity), so that

  * the proof has a closed form over Python integers (closed_form_proof) that shares no DFT, MSM or fold with the library;
  * the sequence the butterflies see can be chosen (families), and what they then meet can be counted by walking the same
    network over the integers (shadow_inverse_dft, shadow_fold): a point is the identity iff its logarithm is 0, two points
    are equal / opposite iff their logarithms are.

Pure Python; the tests that use it are tests/test_degenerate_keys_cpu.py (no GPU: the shadows against direct sums, the closed
form against the oracle, the event counts of every family) and tests/test_gpu_key_degenerate.py."""
import random
from collections import Counter

import numpy as np

import bn254_oracle as o

R = o.R
ACC_LEVEL_L = 8                       # msm.hip: segment length of sum_xyzz_by_key's levels


def inv(x):
    return pow(x % R, R - 2, R)


def dot(u, v):
    return sum(x * y for x, y in zip(u, v)) % R


def scalars(vals):
    return np.frombuffer(b"".join(int(v % R).to_bytes(32, "little") for v in vals), dtype=np.uint8).copy()


# ------------------------------------------------------------------------------------------------- keys
class DlogKey:
    """a, b1, b2: M logarithms each (a_query, b_g1_query, b_g2_query); h: D - 1; l: M - num_inputs; 0 is the identity"""

    def __init__(self, a, b1, b2, h, l, alpha, beta, delta, num_inputs):
        self.a, self.b1, self.b2, self.h, self.l = ([int(x) % R for x in v] for v in (a, b1, b2, h, l))
        self.alpha, self.beta, self.delta, self.num_inputs = alpha % R, beta % R, delta % R, num_inputs
        assert len(self.a) == len(self.b1) == len(self.b2) == len(self.l) + num_inputs
        assert self.alpha and self.beta and self.delta

    def replace(self, **kw):
        d = dict(a=self.a, b1=self.b1, b2=self.b2, h=self.h, l=self.l, alpha=self.alpha, beta=self.beta, delta=self.delta,
                 num_inputs=self.num_inputs)
        d.update(kw)
        return DlogKey(**d)

    def gamma_abc(self):                                  # the prover never reads it; any points will do
        return [1 + i for i in range(self.num_inputs)]


_TABLES = {}


def _g1s(ks):
    if 1 not in _TABLES:
        _TABLES[1] = o.G1.fixed_base_table(o.G1_GEN, 8)
    return o.G1.batch_to_affine([o.G1.fixed_base_mul(_TABLES[1], k % R) for k in ks])


def _g2s(ks):
    if 2 not in _TABLES:
        _TABLES[2] = o.G2.fixed_base_table(o.G2_GEN, 6)
    return o.G2.batch_to_affine([o.G2.fixed_base_mul(_TABLES[2], k % R) for k in ks])


def oracle_key(dl):
    """the oracle's dict form (bn254_oracle.generate_parameters' pk), points made on the CPU"""
    vk = dict(alpha_g1=_g1s([dl.alpha])[0], beta_g2=_g2s([dl.beta])[0], gamma_g2=_g2s([1])[0], delta_g1=_g1s([dl.delta])[0],
              delta_g2=_g2s([dl.delta])[0], gamma_abc_g1=_g1s(dl.gamma_abc()))
    return dict(vk=vk, beta_g1=_g1s([dl.beta])[0], delta_g1=vk["delta_g1"], a_query=_g1s(dl.a), b_g1_query=_g1s(dl.b1),
                b_g2_query=_g2s(dl.b2), h_query=_g1s(dl.h), l_query=_g1s(dl.l))


def proving_key_from_points(cc, pk):
    """cc.ProvingKey from the oracle's dict form"""
    g1 = lambda pts: np.frombuffer(b"".join(o.g1_packed(p) for p in pts), dtype=np.uint8).copy()
    g2 = lambda pts: np.frombuffer(b"".join(o.g2_packed(p) for p in pts), dtype=np.uint8).copy()
    v = pk["vk"]
    vk = cc.VerifyingKey(alpha_g1=g1([v["alpha_g1"]]), beta_g2=g2([v["beta_g2"]]), gamma_g2=g2([v["gamma_g2"]]),
                         delta_g1=g1([v["delta_g1"]]), delta_g2=g2([v["delta_g2"]]), gamma_abc_g1=g1(v["gamma_abc_g1"]))
    return cc.ProvingKey(vk=vk, beta_g1=g1([pk["beta_g1"]]), delta_g1=g1([pk["delta_g1"]]), a_query=g1(pk["a_query"]),
                         b_g1_query=g1(pk["b_g1_query"]), b_g2_query=g2(pk["b_g2_query"]), h_query=g1(pk["h_query"]),
                         l_query=g1(pk["l_query"]))


def gpu_key(cc, dl):
    """cc.ProvingKey with the points made by cc.fixed_base_g1 / fixed_base_g2 (pinned to the oracle by
    test_gpu_parity.py::test_fixed_base_vs_oracle); needs a GPU"""
    f1 = lambda ks: np.frombuffer(bytes(cc.fixed_base_g1(scalars(ks))), dtype=np.uint8).copy() if len(ks) else np.zeros(0, dtype=np.uint8)
    f2 = lambda ks: np.frombuffer(bytes(cc.fixed_base_g2(scalars(ks))), dtype=np.uint8).copy() if len(ks) else np.zeros(0, dtype=np.uint8)
    vk = cc.VerifyingKey(alpha_g1=f1([dl.alpha]), beta_g2=f2([dl.beta]), gamma_g2=f2([1]), delta_g1=f1([dl.delta]),
                         delta_g2=f2([dl.delta]), gamma_abc_g1=f1(dl.gamma_abc()))
    return cc.ProvingKey(vk=vk, beta_g1=f1([dl.beta]), delta_g1=f1([dl.delta]), a_query=f1(dl.a), b_g1_query=f1(dl.b1),
                         b_g2_query=f2(dl.b2), h_query=f1(dl.h), l_query=f1(dl.l))


# ------------------------------------------------------------------------------------------------- the reference
def closed_form_scalars(dl, mats, num_constraints, w, r, s):
    """the logarithms (A, B2, C) of the proof create_proof_with_reduction_and_matrices makes with this key (prover.rs:54-136)"""
    assert w[0] == 1
    l = dl.num_inputs
    h = o.witness_map_from_matrices(mats, l, num_constraints, w)
    A = (dl.alpha + dot(w, dl.a) + r * dl.delta) % R
    B2 = (dl.beta + dot(w, dl.b2) + s * dl.delta) % R
    B1 = (dl.beta + dot(w, dl.b1) + s * dl.delta) % R if r else 0            # prover.rs:102-112
    C = (dot(w[l:], dl.l) + dot(h, dl.h) + s * A + r * B1 - r * s % R * dl.delta) % R     # dot() stops after the D - 1 points
    return A, B2, C


def closed_form_proof(dl, mats, num_constraints, w, r, s):
    """256 bytes: (A·G1, B2·G2, C·G1) as the reference serialises a proof"""
    A, B2, C = closed_form_scalars(dl, mats, num_constraints, w, r % R, s % R)
    g1 = lambda k: o.G1.to_affine(o.G1.mul_affine(o.G1_GEN, k)) if k else None
    return o.proof_uncompressed((g1(A), o.G2.to_affine(o.G2.mul_affine(o.G2_GEN, B2)) if B2 else None, g1(C)))


# ------------------------------------------------------------------------------------------------- shadows
def brev(x, bits):
    return int(bin(x)[2:].zfill(bits)[::-1], 2) if bits else 0


def direct_inverse_dft(x, logn):
    """out[j] = Σ_i ω^{-ij} x_i, by the definition"""
    n = 1 << logn
    wi = inv(o.root_of_unity(n))
    return [sum(pow(wi, i * j % n, R) * x[i] for i in range(n)) % R for j in range(n)]


DFT_EVENTS = ("v_identity", "u_identity_v_finite", "u_eq_t_k0", "u_eq_t_k", "u_eq_neg_t_k0", "u_eq_neg_t_k", "generic")


def shadow_inverse_dft(x, logn):
    """k_ec_load_scale's placement and k_ec_stage's network over logarithms: x[i] is what slot rev(i) holds after the scaling.
    -> (outputs in natural order, Counter of what the butterflies met).  Beside DFT_EVENTS, one per butterfly, the counter
    holds identity_between_stages (identity records a stage stored for the next one to load) and identity_outputs (records
    k_ec_store writes with valid = 0)."""
    n = 1 << logn
    assert len(x) == n
    slots = [0] * n
    for i in range(n):
        slots[brev(i, logn)] = x[i] % R
    wi = inv(o.root_of_unity(n))
    tw = [pow(wi, e, R) for e in range(max(1, n // 2))]
    ev = Counter()
    for q in range(logn):
        half = 1 << q
        for b in range(n >> 1):
            k = b & (half - 1)
            pos = ((b >> q) << (q + 1)) | k
            u, v = slots[pos], slots[pos + half]
            if v == 0:
                ev["v_identity"] += 1
                slots[pos + half] = u
            else:
                t = v if k == 0 else tw[k << (logn - 1 - q)] * v % R
                kk = "k0" if k == 0 else "k"
                if u == 0:
                    ev["u_identity_v_finite"] += 1
                elif u == t:
                    ev["u_eq_t_" + kk] += 1
                elif u == R - t:
                    ev["u_eq_neg_t_" + kk] += 1
                else:
                    ev["generic"] += 1
                slots[pos], slots[pos + half] = (u + t) % R, (u - t) % R
            if q < logn - 1:
                ev["identity_between_stages"] += (slots[pos] == 0) + (slots[pos + half] == 0)
    ev["identity_outputs"] = sum(1 for v in slots if v == 0)
    return slots, ev


def h_scale(logn):
    """k_ec_load_scale's factors for the h transform: g^-i / n"""
    n = 1 << logn
    gi, ninv = inv(o.FR_GENERATOR), inv(n)
    return [ninv * pow(gi, i, R) % R for i in range(n)]


def fold_scale(logn):
    """... for the fold: the constant -vinv / n, vinv = 1 / (g^n - 1)"""
    n = 1 << logn
    return [(R - inv(o.evaluate_vanishing_polynomial(n, o.FR_GENERATOR))) * inv(n) % R] * n


def _scaled(h, scale):
    return [x * s % R for x, s in zip(list(h) + [0] * (len(scale) - len(h)), scale)]


def shadow_h_transform(h, logn):
    """msm.hpp (1): H'_j = Σ_i ω^{-ij}·(g^-i / n)·H_i -> (H', events)"""
    return shadow_inverse_dft(_scaled(h, h_scale(logn)), logn)


def _sum_by_key(keys, vals, M, ev):
    """sum_xyzz_by_key / k_accum_xyzz: segments of ACC_LEVEL_L, a first and a last piece per segment to the next level"""
    sums = [0] * M
    level = 0
    while keys:
        tag = "@0" if level == 0 else "@up"
        cnt = len(keys)
        T = -(-cnt // ACC_LEVEL_L)
        final = T == 1
        nk, nv = [None] * (2 * T), [0] * (2 * T)
        for t in range(T):
            beg = t * ACC_LEVEL_L
            acc, cur, first = 0, keys[beg], True
            for k in range(beg, min(beg + ACC_LEVEL_L, cnt)):
                if keys[k] != cur:
                    if first and not final:
                        nk[2 * t], nv[2 * t] = cur, acc
                        ev["piece_identity" + tag] += acc == 0
                    else:
                        sums[cur] = acc
                    first, acc, cur = False, 0, keys[k]
                q = vals[k]
                if q == 0:
                    ev["add_identity" + tag] += 1
                elif acc == 0:
                    ev["start" + tag] += 1
                elif acc == q:
                    ev["equal" + tag] += 1
                elif acc == R - q:
                    ev["opposite" + tag] += 1
                else:
                    ev["generic" + tag] += 1
                acc = (acc + q) % R
            if final:
                sums[cur] = acc
            elif first:
                nk[2 * t], nv[2 * t], nk[2 * t + 1], nv[2 * t + 1] = cur, acc, cur, 0
                ev["piece_identity" + tag] += acc == 0
                ev["piece_placeholder" + tag] += 1
            else:
                nk[2 * t + 1], nv[2 * t + 1] = cur, acc
                ev["piece_identity" + tag] += acc == 0
        ev["levels"] += 1
        keys, vals = ([], []) if final else (nk, nv)
        level += 1
    return sums


def shadow_fold(h, logn, c_rows, l, num_inputs, M):
    """msm.hpp (2) and ecntt.hip's order of work over logarithms:
         G'_j = -vinv/n · Σ_i ω^{-ij} h_i,   P_k = Σ_j C_jk G'_j,   folded base k = P_k (+ l_{k - num_inputs})
    -> dict(G, P, folded, dft: Counter of shadow_inverse_dft, ev: Counter).  ev counts, for k_ec_terms: term_g_identity,
    term_coeff_zero, term_coeff_one, term_other; for the sums (suffix @0: the level over the terms, @up: the levels over
    pieces): start (the run's accumulator is the identity), add_identity (an identity term or piece is added), equal
    (doubling), opposite (cancellation), generic, piece_identity (a first / last piece that sums to the identity goes up),
    piece_placeholder (the empty last piece of a one-run segment), levels; for k_ec_fold_l, one per wire: fold_p_eq_l,
    fold_p_eq_neg_l, fold_l_identity_p_finite, fold_p_identity_l_finite, fold_both_identity, fold_generic, and
    instance_p_finite / instance_p_identity for the wires below num_inputs."""
    G, dft = shadow_inverse_dft(_scaled(h, fold_scale(logn)), logn)
    ev = Counter()
    cols = [[] for _ in range(M)]                         # csr_transpose: by wire, constraints ascending, a row's terms in order
    for j, row in enumerate(c_rows):
        for coeff, k in row:
            cols[k].append((j, coeff % R))
    keys, vals = [], []
    for k in range(M):
        for j, c in cols[k]:
            if G[j] == 0:
                ev["term_g_identity"] += 1
            elif c == 0:
                ev["term_coeff_zero"] += 1
            elif c == 1:
                ev["term_coeff_one"] += 1
            else:
                ev["term_other"] += 1
            keys.append(k)
            vals.append(c * G[j] % R)
    P = _sum_by_key(keys, vals, M, ev)
    assert P == [sum(c * G[j] for j, c in cols[k]) % R for k in range(M)]
    folded = []
    for k in range(M):
        p = P[k]
        if k < num_inputs:
            ev["instance_p_finite" if p else "instance_p_identity"] += 1
            folded.append(p)
            continue
        lk = l[k - num_inputs]
        if p == 0 and lk == 0:
            ev["fold_both_identity"] += 1
        elif lk == 0:
            ev["fold_l_identity_p_finite"] += 1
        elif p == 0:
            ev["fold_p_identity_l_finite"] += 1
        elif p == lk:
            ev["fold_p_eq_l"] += 1
        elif p == R - lk:
            ev["fold_p_eq_neg_l"] += 1
        else:
            ev["fold_generic"] += 1
        folded.append((p + lk) % R)
    return dict(G=G, P=P, folded=folded, dft=dft, ev=ev)


# ------------------------------------------------------------------------------------------------- circuits
SHAPES = {2: (1, 1, 5), 4: (1, 3, 6), 64: (2, 40, 30), 1024: (2, 1000, 300)}        # D: (l, m, M)
HOT_TERMS = 74                         # terms of the hot C column: more than two levels of ACC_LEVEL_L = 8 (8·8 = 64)


class Circuit:
    """Matrices in the manner of test_gpu_parity.py::test_prove_edge_shapes (rows of 0-3 terms that may repeat a column,
    coefficients 0, 1, r - 1 and random), and in C on purpose:
      hot     a witness wire with HOT_TERMS terms whose coefficients cycle 1, 1, -1, -1: where the G'_j are equal the run
              doubles, returns and cancels every four terms, and a segment of eight sums to the identity;
      absent, absent2   two witness wires with no term in C (P_k the identity);
      zero_coeff        a term with coefficient 0 on wire `plain` (which also has one with 1 and one with r - 1);
      wire 0 and, where there is one, instance wire 1 have terms (finite P_k below num_inputs)."""

    def __init__(self, D, seed=0):
        self.D, self.logn = D, D.bit_length() - 1
        l, m, M = self.l, self.m, self.M = SHAPES[D]
        assert o.domain_size_for(m + l) == D
        rng = random.Random(7000 + 13 * D + seed)
        self.absent, self.absent2, self.hot, self.plain = M - 1, M - 2, M - 3, l
        assert self.plain < self.hot
        coeff = lambda: rng.choice([0, 1, 1, R - 1, rng.randrange(R)])
        row = lambda cols: [(coeff(), rng.choice(cols)) for _ in range(rng.choice([0, 1, 1, 2, 3]))]
        every = list(range(M))
        A, B = [row(every) for _ in range(m)], [row(every) for _ in range(m)]
        in_c = [k for k in every if k not in (self.absent, self.absent2, self.hot)]
        C = [row(in_c) for _ in range(m)]
        p = 0                                            # position in the wire's run: constraints ascending, a row's terms in order
        for j in range(m):                               # spread over the rows, several to a row where the rows are few
            for _ in range(j, HOT_TERMS, m):
                C[j].append(((1, 1, R - 1, R - 1)[p % 4], self.hot))
                p += 1
        C[0] += [(0, self.plain), (1, self.plain), (R - 1, self.plain), (rng.randrange(2, R), 0)]
        C[m - 1] += [(rng.randrange(2, R), self.plain), (1, min(1, l - 1))]
        self.mats = (A, B, C)
        assert sum(1 for r_ in C for _, k in r_ if k == self.hot) == HOT_TERMS
        assert not any(k in (self.absent, self.absent2) for r_ in C for _, k in r_)
        assert all(any(c == want for mat in self.mats for r_ in mat for c, _ in r_) for want in (0, 1, R - 1))

    def matrices(self, cc):
        return cc.ConstraintMatrices.from_rows(self.mats[0], self.mats[1], self.mats[2], self.l, self.M)

    def witnesses(self, seed=0):
        """random non-zero values, and all ones (w[0] = 1 in both)"""
        rng = random.Random(91 + seed)
        return {"random": [1] + [rng.randrange(1, R) for _ in range(self.M - 1)], "ones": [1] * self.M}

    def base_key(self, seed=0):
        """generic a / b / l logarithms with an identity and a repeat in each, and no h query yet"""
        rng = random.Random(555 + seed)
        M, l = self.M, self.l
        a, b, lq = ([rng.randrange(1, R) for _ in range(n)] for n in (M, M, M - l))
        a[M // 2], b[M // 3], lq[0] = 0, 0, 0
        a[1], b[2 % M], lq[1] = a[0], R - b[0], lq[2]
        return DlogKey(a, b, b, [0] * (self.D - 1), lq, *(rng.randrange(1, R) for _ in range(3)), num_inputs=l)


# ------------------------------------------------------------------------------------------------- families
FAMILIES = ("constant", "index0", "index_half", "geometric_low", "geometric_high", "every_second", "half_period", "pair", "two_tone")


def family_sequence(name, logn, seed=0):
    """the n logarithms the butterflies are to see; the last is 0 (the key holds n - 1 points).
      constant        c everywhere
      index0          one point, at index 0
      index_half      one point, at index n/2
      geometric_*     c·ζ^i with ζ = ω^e, e = 3 (below n/2) or n - 5 (above)
      every_second    random at the even indices, the identity at the odd ones
      half_period     x[i + n/2] = x[i] (so x[n/2 - 1] is the identity too): every odd output is the identity
      pair            random, but x[3 + n/2] = x[3], x[6 + n/2] = -x[6], and x[0] such that output 5 is the identity
      two_tone        c·(ω^{3(i+1)} - ω^{(n-5)(i+1)}): all outputs but 3 and n - 5 are the identity (one tone alone would need
                      a point at index n - 1)"""
    n = 1 << logn
    rng = random.Random(4242 + seed + logn)
    c = rng.randrange(1, R)
    if name == "constant":
        x = [c] * n
    elif name == "index0":
        x = [c] + [0] * (n - 1)
    elif name == "index_half":
        assert n >= 4
        x = [0] * n
        x[n // 2] = c
    elif name in ("geometric_low", "geometric_high"):
        assert n >= 16
        z = pow(o.root_of_unity(n), 3 if name == "geometric_low" else n - 5, R)
        x = [c * pow(z, i, R) % R for i in range(n)]
    elif name == "every_second":
        x = [rng.randrange(1, R) if i % 2 == 0 else 0 for i in range(n)]
    elif name == "half_period":
        assert n >= 8
        x = [rng.randrange(1, R) for _ in range(n // 2 - 1)] + [0]
        x = x + x
    elif name == "two_tone":
        assert n >= 16
        w = o.root_of_unity(n)
        x = [c * (pow(w, 3 * (i + 1) % n, R) - pow(w, (n - 5) * (i + 1) % n, R)) % R for i in range(n)]
        assert x[n - 1] == 0
    elif name == "pair":
        assert n >= 16
        x = [rng.randrange(1, R) for _ in range(n)]
        x[3 + n // 2], x[6 + n // 2] = x[3], R - x[6]
        x[n - 1] = 0
        wi = inv(o.root_of_unity(n))
        x[0] = (R - sum(pow(wi, 5 * i % n, R) * x[i] for i in range(1, n))) % R
    else:
        raise ValueError(name)
    x[n - 1] = 0
    return x


def family_h(name, aim, logn, seed=0):
    """the D - 1 h-query logarithms for which the transform `aim` ("h": ec_transform_h_bases, "fold": the fold's) sees
    family_sequence(name) after k_ec_load_scale's factor"""
    scale = h_scale(logn) if aim == "h" else fold_scale(logn)
    x = family_sequence(name, logn, seed)
    return [v * inv(s) % R for v, s in zip(x, scale)][:-1]


def generic_h(logn, seed=0):
    rng = random.Random(77 + seed)
    return [rng.randrange(1, R) for _ in range((1 << logn) - 1)]


def aimed_l(circ, key):
    """the l query aimed at k_ec_fold_l, from the P_k of the key's own h query: per witness wire
         first      l = P       (madd29's doubling branch)
         second     l = -P      (the folded base is the identity)
         third      l = identity, P finite
         absent     l finite, P identity;   absent2: both the identity
       the others as they were -> (key with that l query, {role: wire})"""
    f = shadow_fold(key.h, circ.logn, circ.mats[2], key.l, circ.l, circ.M)
    l = circ.l
    free = [k for k in range(l, circ.M) if f["P"][k] and k != circ.hot]
    assert len(free) >= 3
    roles = dict(doubling=free[0], cancelling=free[1], l_identity=free[2], p_identity=circ.absent, both_identity=circ.absent2)
    lq = list(key.l)
    lq[roles["doubling"] - l] = f["P"][roles["doubling"]]
    lq[roles["cancelling"] - l] = R - f["P"][roles["cancelling"]]
    lq[roles["l_identity"] - l] = 0
    lq[circ.absent2 - l] = 0
    assert lq[circ.absent - l]
    return key.replace(l=lq), roles


# ------------------------------------------------------------------------------------------------- the cases of the GPU file
# name: (D, family, the transform it is aimed at).  index0, index_half and every_second are the same kind of sequence for both
# transforms (a factor per point changes no identity), so one key serves both.
CASES = {
    "constant/h": (64, "constant", "h"), "constant/fold": (64, "constant", "fold"),
    "index0": (64, "index0", "h"), "index_half": (64, "index_half", "h"),
    "geometric_low/h": (64, "geometric_low", "h"), "geometric_high/fold": (64, "geometric_high", "fold"),
    "every_second": (64, "every_second", "h"),
    "half_period/h": (64, "half_period", "h"), "half_period/fold": (64, "half_period", "fold"),
    "pair/h": (64, "pair", "h"), "pair/fold": (64, "pair", "fold"),
    "two_tone/h": (64, "two_tone", "h"), "two_tone/fold": (64, "two_tone", "fold"),
    "aimed_l": (64, None, None),
    "D2/index0": (2, "index0", "h"), "D4/constant": (4, "constant", "h"),
    "D1024/two_tone/h": (1024, "two_tone", "h"), "D1024/two_tone/fold": (1024, "two_tone", "fold"),
}


def case_key(name):
    """-> (Circuit, DlogKey, roles of aimed_l or None)"""
    D, family, aim = CASES[name]
    circ = Circuit(D)
    key, roles = circ.base_key(), None
    if family is None:
        key, roles = aimed_l(circ, key.replace(h=generic_h(circ.logn)))
    else:
        key = key.replace(h=family_h(family, aim, circ.logn))
    if name == "two_tone/fold":                  # nearly every P_k is the identity; with this l query so is the folded table
        key = key.replace(l=[v if i in (3, 4, 11) else 0 for i, v in enumerate(key.l)])
    return circ, key, roles


def case_events(name):
    """-> (H', events of the h transform, shadow_fold's result) for the key of a case"""
    circ, key, _ = case_key(name)
    return shadow_h_transform(key.h, circ.logn) + (shadow_fold(key.h, circ.logn, circ.mats[2], key.l, circ.l, circ.M),)
