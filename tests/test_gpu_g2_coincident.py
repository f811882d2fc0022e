"""Coincident and opposite points in BOTH G2 bucket accumulations.  Needs an MI355X.

The mixed addition of the G2 accumulation exists twice on the device only: over a lane pair (csrc/g2pair.hpp pr_madd, run by
k_accum_affine_g2_pair in every latency engine) and on one lane with the accumulator in LDS (msm.hip madd29_lds, run by
k_accum_affine_g2 in throughput engines).  Both branch when the incoming table point has the x of the running sum: equal y is a
doubling (pr_dbl_affine / dbl_affine29), opposite y the identity, after which the run restarts.  Distinct random bases never
get there, and tests/cpp/test_field29.cpp can compile neither of the two.  Here the bases coincide on purpose:

  1. MsmContext(group=2) - the pair kernel - over ONE base repeated, P and -P alternating, and P, 2P, -P cycling, against the
     closed form (Σ s_i k_i mod r)·G2 in Python integers;
  2. the prover over keys whose b_g2_query (and, for two of them, a_query and b_g1_query) repeats one point and its negative,
     as two wires with the same B column do in a real key, on a latency context (pair kernel), a one-slot throughput context
     and a three-slot one (LDS kernel), against oracle/cpu_ref.c, which takes any key.

Every comparison is of bytes."""
import copy
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


def _scalars(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).copy()


# ------------------------------------------------------------------------- 1. the pair kernel through MsmContext(group=2)
# odd; 2501 one-digit entries in 16-entry latency segments are 157 segments: three waves of k_combine_wave, then a second level.
# (4001 made the c = 3 case, 85 window rows a base, cost three times the G1 rare-branch test's longest case.)
N_BASES = 2501


def _default_window(n):
    """msm.hip msm_default_window(n, precomputed = true), restated: the window a resident-table context takes for window_bits = 0"""
    best, best_c = None, 4
    for c in range(4, 23):
        W = (255 + c - 1) // c
        cost = n * W * 12.0 + (1 << (c - 1)) * 2.0 * 16.0
        if best is None or cost < best:
            best, best_c = cost, c
    return best_c


@pytest.mark.parametrize("wb", [3, 8, 14, 0])
def test_pair_kernel_same_x_branches_against_the_closed_form(cc, oracle, wb):
    """The G2 counterpart of test_gpu_parity.py::test_signed_accumulation_rare_branches_on_the_gpu.  A run made only of copies of
    P cannot get from P to 3P without P + P: "one base, ones" doubles in every one of its 157 segments, and the equal pieces the
    segments leave meet again in the combine levels.  A bucket holding only P and -P decides at its second entry between
    doubling and cancellation, and the run restarts after a cancellation.  half - 1 and half + 1 recode to one digit magnitude
    with opposite signs, so pr_load_coord's negation meets the same base.  "ones, the last 0" over P and -P is 1250 of each: the
    total is the identity and the result must be 128 zero bytes.  Narrow, medium, wide and default windows; every case twice
    on one handle (buckets and counters left clean)."""
    rng = random.Random(909 + wb)
    n = N_BASES
    R = oracle.R
    k0 = rng.randrange(1, R)
    bases_sets = {
        "one base": [k0] * n,
        "P and -P": [k0 if i & 1 else R - k0 for i in range(n)],
        "P, 2P, -P": [(k0, 2 * k0 % R, R - k0)[i % 3] for i in range(n)],
    }
    half = 1 << ((wb or _default_window(n)) - 1)
    pops = {
        "ones": [1] * n,
        "minus ones": [R - 1] * n,
        "same digit both signs": [(half - 1) if i & 1 else (half + 1) for i in range(n)],
        "5 and r - 5": [5 if i % 3 else R - 5 for i in range(n)],
        "uniform": [rng.randrange(R) for _ in range(n)],
        "ones, the last 0": [1] * (n - 1) + [0],
    }
    identities = 0
    for bname, ks in bases_sets.items():
        bases = cc.fixed_base_g2(_scalars(ks))
        ctx = cc.MsmContext(bases, group=2, window_bits=wb)
        try:
            for pname, sc in pops.items():
                e = sum(k * s_ for k, s_ in zip(ks, sc)) % R
                exp = oracle.g2_packed(oracle.G2.to_affine(oracle.G2.mul_affine(oracle.G2_GEN, e))) if e else bytes(128)
                identities += e == 0
                arr = _scalars(sc)
                assert ctx.run(arr) == exp, (wb, bname, pname)
                assert ctx.run(arr) == exp, (wb, bname, pname, "second run")
        finally:
            ctx.close()
    assert identities >= 1                                           # a total that cancels was among them


# ------------------------------------------------------------ 2. both kernels through the prover, keys with repeated B points
L_, M_, V_ = 6, 3_000, 3_100          # D = 2^12; the G2 MSM has thousands of entries: many segments of 16 and of 64 (asserted below)


def _rewrite(query, size, choose):
    """a copy of a packed query in which every NON-identity point i becomes P (choose(i) = 1), -P (-1) or stays (0); P is the
    first non-identity point; -P negates every component of y (q - v, 0 stays 0); identity entries stay identity"""
    import bn254_oracle as o
    q = query.copy()
    pts = q.reshape(-1, size)
    live = np.flatnonzero(pts.any(axis=1))
    P = pts[live[0]].copy()
    negP = P.copy()
    for k in range(size // 2, size, 32):
        v = int.from_bytes(P[k:k + 32].tobytes(), "little")
        negP[k:k + 32] = np.frombuffer(((o.Q - v) % o.Q).to_bytes(32, "little"), dtype=np.uint8)
    for i in live:
        c = choose(int(i))
        if c:
            pts[i] = P if c > 0 else negP
    return q


_ALL_P = lambda i: 1
_ALTERNATE = lambda i: 1 if i & 1 else -1
_THIRDS = lambda i: (1, -1, 0)[i % 3]


class _Keys:
    """the circuit, its two assignments, the honest key, the derived keys and - computed once per key - the expected proofs"""

    def __init__(self, cc, oracle):
        from crescent_credentials_amd import workloads as wl
        self.cm, w_sat = wl.synthetic_circuit(2606, L_, M_, V_, 0.9, 3, profile="gates")
        rng = random.Random(2606)
        self.pk = cc.generate_parameters_with_qap(self.cm, *(rng.randrange(1, oracle.R) for _ in range(4)))
        w_any = _scalars([rng.randrange(oracle.R) for _ in range(V_)])
        self.rs = [(0, 0), (0, 5), (rng.randrange(1, oracle.R), rng.randrange(1, oracle.R))]
        self.jobs = [(w, r, s) for w in (w_sat, w_any) for r, s in self.rs]       # the first three: the satisfying, 0/1-heavy witness
        self._keys, self._want = {}, {}

    def key(self, name):
        if name not in self._keys:
            pk = self.pk
            k = copy.copy(pk)
            choose = {"a": _ALL_P, "b": _ALTERNATE, "c": _THIRDS, "d_a": _ALL_P, "d_b": _ALTERNATE}[name]
            k.b_g2_query = _rewrite(pk.b_g2_query, 128, choose)
            if name.startswith("d_"):
                k.b_g1_query = _rewrite(pk.b_g1_query, 64, choose)
                k.a_query = _rewrite(pk.a_query, 64, choose)
            # the identity pattern is untouched, and b_g1 / b_g2 still share it
            z2 = ~k.b_g2_query.reshape(-1, 128).any(axis=1)
            assert (z2 == ~pk.b_g2_query.reshape(-1, 128).any(axis=1)).all() and (z2 == ~k.b_g1_query.reshape(-1, 64).any(axis=1)).all()
            assert (~z2).sum() > 100
            self._keys[name] = k
        return self._keys[name]

    def want(self, name):
        if name not in self._want:
            import cpu_ref
            cm = self.cm
            self._want[name] = [cpu_ref.prove(self.key(name), (cm.a, cm.b, cm.c), L_, M_, V_, w, r, s, nthreads=8) for w, r, s in self.jobs]
        return self._want[name]


@pytest.fixture(scope="module")
def keys(cc, oracle):
    return _Keys(cc, oracle)


def test_the_derived_keys_are_what_they_claim(keys, oracle):
    """(a) one point everywhere, (b) P / -P by wire parity with -P = (x, -y) on the curve, (c) a third P, a third -P, the rest
    kept; (d) the same in a_query and b_g1_query from their own first points"""
    pk = keys.pk
    for name, field, size in (("a", "b_g2_query", 128), ("d_a", "b_g1_query", 64), ("d_a", "a_query", 64)):
        pts = getattr(keys.key(name), field).reshape(-1, size)
        assert len({bytes(p) for p in pts[pts.any(axis=1)]}) == 1
    b = keys.key("b").b_g2_query.reshape(-1, 128)
    live = np.flatnonzero(b.any(axis=1))
    P, nP = (oracle.g2_unpack(bytes(b[[i for i in live if i & 1 == par][0]])) for par in (1, 0))
    assert P == oracle.g2_unpack(bytes(pk.b_g2_query.reshape(-1, 128)[live[0]]))
    assert nP[0] == P[0] and all((u + v) % oracle.Q == 0 for u, v in zip(P[1], nP[1])) and nP != P
    assert oracle.G2.is_on_curve(P) and oracle.G2.is_on_curve(nP) and nP == oracle.G2.neg_affine(P)
    assert {bytes(b[i]) for i in live if i & 1} == {oracle.g2_packed(P)} and {bytes(b[i]) for i in live if not i & 1} == {oracle.g2_packed(nP)}
    c = keys.key("c").b_g2_query.reshape(-1, 128)
    kept = [i for i in live if i % 3 == 2]
    assert all(bytes(c[i]) == bytes(pk.b_g2_query.reshape(-1, 128)[i]) for i in kept) and len(kept) > 30
    assert {bytes(c[i]) for i in live if i % 3 == 0} == {oracle.g2_packed(P)} and {bytes(c[i]) for i in live if i % 3 == 1} == {oracle.g2_packed(nP)}


_CONTEXTS = {
    # name: (Prover arguments, latency_mode, lone slots, shortest segment of the accumulation, callers)
    "latency_pair_kernel": (dict(), 1, 0, 16, 1),
    "throughput_one_slot_lds_kernel": (dict(proof_slots=1, mode="throughput"), 0, 0, 64, 1),
    "three_slots_lds_kernel": (dict(proof_slots=3, lone_slot=False), 0, 0, 64, 3),
}


@pytest.mark.parametrize("context", list(_CONTEXTS))
@pytest.mark.parametrize("key", ["a", "b", "c", "d_a", "d_b"])
def test_proofs_over_keys_with_repeated_b_points(cc, oracle, keys, key, context):
    """The satisfying witness is 0/1-heavy: the rewritten points of its one-wires share bucket 1 of the G2 MSM, which is then a
    run of P's (key a: a doubling in every segment), a walk over P and -P (b: doublings of either sign and cancellations; its
    share of the B part of the proof cancels all but a few), or those among other points (c).  Keys d put a bucket set holding
    a single point, and one whose total cancels, through the G1 accumulation and reductions as well - on the one-stream
    throughput slot through the batched chain.  The uniform assignment spreads the same points over every bucket and window
    row.  (r, s) = (0, 0), (0, 5) - no b1 MSM - and a random pair; every proof twice, before and after the one-time window
    re-tune; the three-slot context is driven by three callers at once."""
    kw, latency_mode, lone, min_segment, callers = _CONTEXTS[context]
    k = keys.key(key)
    want = keys.want(key)
    prover = cc.Prover(k, keys.cm, **kw)
    try:
        i = prover.info()
        assert i["latency_mode"] == latency_mode and i["lone_slots"] == lone and i["proof_slots"] == kw.get("proof_slots", 1)
        for rnd in range(2):
            if callers == 1:
                got = [prover.prove(*j).data for j in keys.jobs]
            else:
                with ThreadPoolExecutor(max_workers=callers) as ex:
                    got = list(ex.map(lambda j: prover.prove(*j).data, keys.jobs))
            for n, (g, e) in enumerate(zip(got, want)):
                assert g == e, (key, context, "round %d" % rnd, "witness" if n < 3 else "uniform assignment", keys.rs[n % 3][0] == 0)
        # the accumulation was cut into many segments (the satisfying witness is the one with the fewest entries)
        proof, tm = prover.prove(*keys.jobs[2], timings=True)
        assert proof.data == want[2]
        assert tm["entries_g2"] > 4 * min_segment, tm["entries_g2"]
    finally:
        prover.close()
