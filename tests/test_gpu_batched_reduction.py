"""The batched tail of a proof on a one-stream slot: the l, a, b1 and h MSMs leave their buckets un-reduced and ONE chain of
three launches reduces the four bucket sets (msm.hip enqueue_reduction_batch).  Needs an MI355X.

Every comparison is of proof bytes.  The references: oracle/bn254_oracle.py itself at D = 2^10 (about four seconds a proof),
and at D = 2^11 - 2^12, where it takes a quarter of a minute a proof, oracle/cpu_ref.c, the oracle's C restatement that
tests/test_cpu_ref.py pins to it; and a latency context (five streams: every MSM reduces its own buckets) on the same input.
Throughput contexts here are loaded with lone_slot=False: a proof that arrives alone would otherwise run on the lone slot,
which does not batch."""
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L12, M12, V12 = 6, 4_000, 4_060         # D = 2^12


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


def _key(cc, oracle, cm, seed):
    rng = random.Random(seed)
    tau, alpha, beta, delta = (rng.randrange(1, oracle.R) for _ in range(4))
    return cc.generate_parameters_with_qap(cm, alpha, beta, delta, tau)


def _random_assignment(nprng, M, zero_from=None):
    a = nprng.integers(0, 256, (M, 32), dtype=np.uint8)
    a[:, 31] %= 0x30                                    # canonical
    if zero_from is not None:
        a[zero_from:] = 0
    a[0] = 0
    a[0, 0] = 1                                         # the constant-one wire
    return a.reshape(-1).copy()


@pytest.fixture(scope="module")
def d12(cc, oracle):
    """one circuit at D = 2^12 with a bit-heavy (0.9) and an all-uniform assignment of its shape, and its key"""
    from crescent_credentials_amd import workloads as wl
    cm, w_bits = wl.synthetic_circuit(812, L12, M12, V12, 0.9, 3)
    _, w_uniform = wl.synthetic_circuit(813, L12, M12, V12, 0.0, 3)
    return cm, _key(cc, oracle, cm, 12), w_bits, w_uniform


def _ref(d, w, r, s):
    import cpu_ref
    cm, pk = d[0], d[1]
    return cpu_ref.prove(pk, (cm.a, cm.b, cm.c), cm.num_instance_variables, cm.num_constraints, cm.num_variables, w, r, s, nthreads=8)


def _geometry(c):
    """(R, C) of the bucket matrix of a window of c bits (msm.hip red_cbits)"""
    cbits = min(10, c // 2)
    return (1 << (c - 1)) >> cbits, 1 << cbits


def _g1_geometries(prover):
    wb = prover.info()["window_bits"]
    return [_geometry(wb[k]) for k in ("h", "l", "a", "b_g1")]


def test_bucket_sets_of_different_shapes_in_one_batch_python_oracle(cc, oracle):
    """D = 2^10 against bn254_oracle.py: the size-based windows first, then, after the re-tune that the first proof of a
    bit-heavy witness triggers, narrower windows for l / a / b1 than for h - bucket matrices of different (R, C) in one
    batch (R != C is the next test's)."""
    from crescent_credentials_amd import workloads as wl
    l, m, M = 4, 1_000, 1_010
    cm, w = wl.synthetic_circuit(810, l, m, M, 0.9, 3)
    pk = _key(cc, oracle, cm, 10)
    def rows(csr):
        co = bytes(csr.coeff)
        return [[(int.from_bytes(co[32 * k:32 * k + 32], "little"), int(csr.col[k])) for k in range(int(csr.row_ptr[i]), int(csr.row_ptr[i + 1]))]
                for i in range(m)]
    mats = (rows(cm.a), rows(cm.b), rows(cm.c))
    g1 = lambda a: [oracle.g1_unpack(bytes(a[i:i + 64])) for i in range(0, a.size, 64)]
    g2 = lambda a: [oracle.g2_unpack(bytes(a[i:i + 128])) for i in range(0, a.size, 128)]
    pk_o = dict(vk=dict(alpha_g1=g1(pk.vk.alpha_g1)[0], beta_g2=g2(pk.vk.beta_g2)[0], delta_g2=g2(pk.vk.delta_g2)[0]),
                beta_g1=g1(pk.beta_g1)[0], delta_g1=g1(pk.delta_g1)[0], a_query=g1(pk.a_query), b_g1_query=g1(pk.b_g1_query),
                b_g2_query=g2(pk.b_g2_query), h_query=g1(pk.h_query), l_query=g1(pk.l_query))
    rng = random.Random(1010)
    r, s = rng.randrange(1, oracle.R), rng.randrange(oracle.R)
    wi = [int.from_bytes(bytes(w[i:i + 32]), "little") for i in range(0, w.size, 32)]
    want = oracle.proof_uncompressed(oracle.create_proof_with_reduction_and_matrices(pk_o, r, s, mats, l, m, wi))
    thr = cc.Prover(pk, cm, proof_slots=2, mode="throughput", lone_slot=False)
    lat = cc.Prover(pk, cm, mode="latency")
    try:
        assert thr.info()["latency_mode"] == 0 and thr.info()["lone_slots"] == 0
        assert thr.prove(w, r, s).data == want                     # size-based windows; its statistics re-tune the context
        assert thr.info()["tuned"] == 1
        geo = _g1_geometries(thr)
        print("windows", thr.info()["window_bits"], "bucket matrices (h, l, a, b1)", geo)
        assert len(set(geo)) >= 2
        assert thr.prove(w, r, s).data == want
        assert lat.prove(w, r, s).data == want
    finally:
        thr.close(); lat.close()


@pytest.mark.parametrize("window_bits", [0, 12, 16], ids=["retuned", "c12", "c16"])
def test_bucket_sets_of_different_shapes_in_one_batch(cc, oracle, d12, window_bits):
    """D = 2^12.  Re-tuned windows: h keeps c = 13 (64 x 64 buckets, four tiles, a workgroup) next to the narrower, odd c - 1
    windows of the bit-heavy a / b1.  c = 12: 32 x 64 for every engine (R != C, two tiles a job, so job boundaries inside
    the launch fall on single workgroups).  c = 16: 128 x 256, 32 tiles and eight workgroups a job."""
    cm, pk, w, _ = d12
    rng = random.Random(1200 + window_bits)
    rs = [(rng.randrange(1, oracle.R), rng.randrange(oracle.R)) for _ in range(2)]
    want = [_ref(d12, w, r, s) for r, s in rs]
    thr = cc.Prover(pk, cm, proof_slots=2, mode="throughput", lone_slot=False, window_bits=window_bits)
    lat = cc.Prover(pk, cm, mode="latency", window_bits=window_bits)
    try:
        assert thr.prove(w, *rs[0]).data == want[0]
        geo = _g1_geometries(thr)
        print("windows", thr.info()["window_bits"], "bucket matrices (h, l, a, b1)", geo)
        if window_bits == 0:
            assert thr.info()["tuned"] == 1
            assert len(set(geo)) >= 2 and any(R != C for R, C in geo)
        elif window_bits == 12:
            assert set(geo) == {(32, 64)}
        assert thr.prove(w, *rs[1]).data == want[1]
        assert [lat.prove(w, r, s).data for r, s in rs] == want
    finally:
        thr.close(); lat.close()


def test_buckets_and_counters_are_left_clean(cc, oracle, d12):
    """three proofs one after another on the same slot (one caller: always the first slot), different assignments and (r, s):
    a bucket or a partition counter that the batched chain left dirty would corrupt the second"""
    cm, pk, w_bits, w_uniform = d12
    nprng = np.random.default_rng(3)
    rng = random.Random(33)
    cases = [(w_bits, rng.randrange(1, oracle.R), rng.randrange(oracle.R)), (_random_assignment(nprng, V12), rng.randrange(1, oracle.R), 0),
             (w_uniform, rng.randrange(1, oracle.R), rng.randrange(oracle.R))]
    thr = cc.Prover(pk, cm, proof_slots=2, mode="throughput", lone_slot=False)
    try:
        for k, (w, r, s) in enumerate(cases):
            assert thr.prove(w, r, s).data == _ref(d12, w, r, s), k
    finally:
        thr.close()


@pytest.mark.parametrize("h_coefficient_basis", [False, True], ids=["folded", "plain"])
def test_engines_that_drop_out_of_the_batch(cc, oracle, d12, h_coefficient_basis):
    """r = 0 (no b1 MSM: three jobs); every wire but the constant zero (l, a, b1 run with no entry at all - over the plain key;
    over the folded key l has the constant wire's one); then a full batch again on the same slot"""
    cm, pk, w_bits, _ = d12
    nprng = np.random.default_rng(4)
    rng = random.Random(44)
    r, s = rng.randrange(1, oracle.R), rng.randrange(oracle.R)
    w_zero = _random_assignment(nprng, V12, zero_from=1)
    thr = cc.Prover(pk, cm, proof_slots=2, mode="throughput", lone_slot=False, h_coefficient_basis=h_coefficient_basis)
    try:
        for k, (w, rr, ss) in enumerate([(w_bits, 0, s), (w_bits, r, s), (w_zero, r, s), (w_zero, 0, 0), (w_bits, r, s)]):
            assert thr.prove(w, rr, ss).data == _ref(d12, w, rr, ss), k
    finally:
        thr.close()


def test_an_l_query_of_a_handful_of_wires(cc, oracle):
    """M - l = 5 witness wires under 1000 instance wires (D = 2^11): over the plain key the l engine has five bases, and
    over the folded key one per wire"""
    import cpu_ref
    l, m, M = 1_000, 1_000, 1_005
    rng = random.Random(55)
    row = lambda: [(rng.randrange(oracle.R), rng.randrange(M)) for _ in range(rng.choice([1, 2, 3]))]
    mats = tuple([row() for _ in range(m)] for _ in range(3))
    cm = cc.ConstraintMatrices.from_rows(mats[0], mats[1], mats[2], l, M)
    pk = _key(cc, oracle, cm, 5)
    nprng = np.random.default_rng(5)
    w = _random_assignment(nprng, M)
    rs = [(rng.randrange(1, oracle.R), rng.randrange(oracle.R)), (0, rng.randrange(oracle.R))]
    want = [cpu_ref.prove(pk, (cm.a, cm.b, cm.c), l, m, M, w, r, s, nthreads=8) for r, s in rs]
    for plain in (True, False):
        thr = cc.Prover(pk, cm, proof_slots=2, mode="throughput", lone_slot=False, h_coefficient_basis=plain)
        try:
            assert [thr.prove(w, r, s).data for r, s in rs] == want, plain
        finally:
            thr.close()


@pytest.mark.parametrize("which", ["bit_heavy", "uniform"])
def test_run_lengths_and_edge_tiles(cc, oracle, d12, which):
    """a bit-heavy witness (long runs in few buckets, narrow re-tuned windows: partial tiles) and an all-uniform one (short
    runs in every bucket), before and after the re-tune"""
    cm, pk, w_bits, w_uniform = d12
    w = w_bits if which == "bit_heavy" else w_uniform
    rng = random.Random(66)
    rs = [(rng.randrange(1, oracle.R), rng.randrange(oracle.R)) for _ in range(3)]
    thr = cc.Prover(pk, cm, proof_slots=2, mode="throughput", lone_slot=False)
    try:
        assert [thr.prove(w, r, s).data for r, s in rs] == [_ref(d12, w, r, s) for r, s in rs]
        print("windows", thr.info()["window_bits"], "bucket matrices (h, l, a, b1)", _g1_geometries(thr))
    finally:
        thr.close()


def test_concurrent_callers(cc, oracle, d12):
    """four callers on a four-slot context, 32 proofs (every fourth with r = 0): each equals the bytes of a one-slot latency
    context"""
    cm, pk, w_bits, w_uniform = d12
    rng = random.Random(77)
    jobs = [((w_bits, w_uniform)[k % 2], 0 if k % 4 == 3 else rng.randrange(1, oracle.R), rng.randrange(oracle.R)) for k in range(32)]
    lat = cc.Prover(pk, cm, mode="latency")
    thr = cc.Prover(pk, cm, proof_slots=4, mode="throughput", lone_slot=False)
    try:
        want = [lat.prove(w, r, s).data for w, r, s in jobs]
        assert want[0] == _ref(d12, *jobs[0]) and want[3] == _ref(d12, *jobs[3])
        with ThreadPoolExecutor(max_workers=4) as ex:
            got = list(ex.map(lambda j: thr.prove(*j).data, jobs))
        assert got == want
    finally:
        lat.close(); thr.close()


def test_timings_of_a_batched_proof(cc, oracle, d12):
    """msm_h_ms carries the batched chain (h is the last MSM of the stream) and the other three end with their combine levels;
    the entry and pair counts are those of a latency context with the same windows"""
    cm, pk, w, _ = d12
    rng = random.Random(88)
    r, s = rng.randrange(1, oracle.R), rng.randrange(oracle.R)
    thr = cc.Prover(pk, cm, proof_slots=2, mode="throughput", lone_slot=False, window_bits=12)
    lat = cc.Prover(pk, cm, mode="latency", window_bits=12)
    try:
        thr.prove(w, r, s)
        p, tm = thr.prove(w, r, s, timings=True)
        q, tl = lat.prove(w, r, s, timings=True)
        print({k: tm[k] for k in ("msm_h_ms", "msm_l_ms", "msm_a_ms", "msm_b1_ms", "msm_b2_ms", "accum_g1_ms", "sort_ms")})
        assert p.data == q.data == _ref(d12, w, r, s)
        assert tm["msm_h_ms"] > 0
        assert tm["msm_h_ms"] >= max(tm["msm_l_ms"], tm["msm_a_ms"], tm["msm_b1_ms"])
        assert min(tm["msm_l_ms"], tm["msm_a_ms"], tm["msm_b1_ms"]) > 0
        assert tm["entries_g1"] == tl["entries_g1"] > 0 and tm["msm_g1_pairs"] == tl["msm_g1_pairs"] > 0
    finally:
        thr.close(); lat.close()
