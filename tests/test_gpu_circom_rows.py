"""Long, repeated and hot-column R1CS rows on the GPU, against oracle/cpu_ref.c and the Python oracle, byte for byte.

The instances (tests/circom_rows.py) carry rows at every boundary of the sliced sparse product (wmap29.hip k_sell29, up to
8 levels of 8-term pieces), transposed columns of exactly 4096 and 4097 terms (the setup's k_spmv / k_spmv_long split in
ntt.hip), a wire repeated hundreds of times in one row and pairs c, r - c on one (row, wire) (the doubling and cancelling
branches of the G1 C fold only, ecntt.hip k_ec_terms + msm.hip sum_xyzz_by_key; the same-x branches of the G2 bucket
accumulations are tests/test_gpu_g2_coincident.py's), and a row of exactly 8^8 terms, the longest the layout holds.  Two sizes: SMALL (D = 2^8) where the Python oracle is affordable, MEDIUM (D = 2^17, ~3.8 M terms, a
dictionary of more than 2^20 coefficients in A)."""
import hashlib
import random

import numpy as np
import pytest

import circom_rows as cr

pytestmark = pytest.mark.gpu

SMALL = (4, 200, 300)                   # l, m, M: D = 256, every row boundary up to 262145 terms
MEDIUM = (20, 131_000, 133_000)         # D = 2^17
NT = 16


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


def _cm(cc, inst):
    A, B, C = inst.mats
    return cc.ConstraintMatrices(A, B, C, inst.l, inst.M - inst.l, inst.m)


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _digest(pk):
    return [_sha(x) for x in (pk.vk.alpha_g1, pk.beta_g1, pk.delta_g1, pk.vk.beta_g2, pk.vk.gamma_g2, pk.vk.delta_g2,
                              pk.vk.gamma_abc_g1, pk.a_query, pk.b_g1_query, pk.b_g2_query, pk.h_query, pk.l_query)]


def _witnesses(inst):
    """random (satisfying), all-zero, all-(r-1), and two whose longest rows of A / B come out exactly 0 / r - 1"""
    big = inst.rows["len%d" % max(int(k[3:]) for k in inst.rows if k.startswith("len"))]
    return {"random": inst.w, "zeros": cr.extreme_witness(inst, "zeros"), "max": cr.extreme_witness(inst, "max"),
            "row0": cr.extreme_witness(inst, "row", np.random.default_rng(3), (0, big), 0),
            "rowmax": cr.extreme_witness(inst, "row", np.random.default_rng(4), (1, big), cr.R - 1)}


@pytest.fixture(scope="module")
def small():
    return cr.circom_instance(*SMALL, seed=11)


@pytest.fixture(scope="module")
def medium():
    return cr.circom_instance(*MEDIUM, seed=12, hot_terms=20_000, mixes=(cr.MIX_DICT_HEAVY, cr.MIX_CIRCOM, cr.MIX_CIRCOM),
                              dict_size=(None, 4096, 4096), nthreads=NT)


@pytest.fixture(scope="module")
def small_key(cc, small):
    alpha, beta, delta, tau = _trap(5)
    return cc.generate_parameters_with_qap(_cm(cc, small), alpha, beta, delta, tau), (alpha, beta, delta, tau)


def _trap(seed):
    rng = random.Random(seed)
    return [rng.randrange(1, cr.R) for _ in range(4)]           # alpha, beta, delta, tau


@pytest.fixture(scope="module")
def medium_key(cc, medium):
    alpha, beta, delta, tau = _trap(21)
    pk = cc.generate_parameters_with_qap(_cm(cc, medium), alpha, beta, delta, tau)
    return pk, (alpha, beta, delta, tau)


# ------------------------------------------------------------------------------------------- witness map
@pytest.mark.parametrize("size", ["small", "medium"])
def test_witness_map_every_entry(cc, oracle, request, size):
    """h of every witness kind through Prover.witness_map, QapContext (host and device buffers) and
    LibsnarkReduction.witness_map_from_matrices == cpu_ref.witness_map (and the Python oracle on the small instance)"""
    import cpu_ref
    import torch
    inst = request.getfixturevalue(size)
    cm = _cm(cc, inst)
    l, m, M = inst.l, inst.m, inst.M
    pk = request.getfixturevalue(size + "_key")[0]
    prover = cc.Prover(pk, cm)
    qap = cc.QapContext(cm)
    rows = inst.to_rows() if size == "small" else None
    try:
        for name, w in _witnesses(inst).items():
            want = bytes(cpu_ref.witness_map(inst.mats, l, m, M, w, nthreads=NT))
            if rows is not None:
                assert want == bytes(cr.fr_bytes(oracle.witness_map_from_matrices(rows, l, m, cr.ints_of(w)))), name
            assert bytes(prover.witness_map(w)) == want, ("Prover", name)
            assert bytes(qap.witness_map(w)) == want, ("QapContext", name)
            wd = torch.from_numpy(np.ascontiguousarray(w)).cuda()
            hd = torch.zeros(qap.domain_size * 32, dtype=torch.uint8, device="cuda")
            qap.witness_map_dev(wd.data_ptr(), hd.data_ptr())
            torch.cuda.synchronize()
            assert bytes(hd.cpu().numpy()) == want, ("QapContext device", name)
            assert bytes(cc.LibsnarkReduction.witness_map_from_matrices(cm, l, m, w)) == want, ("LibsnarkReduction", name)
    finally:
        prover.close()
        qap.close()
        cc.LibsnarkReduction.clear_cache()


# ------------------------------------------------------------------------------------------- coset forms
def test_coset_values_and_shards(cc, medium, medium_key):
    """witness_map_coset / _half == vinv·a(gω^j)·b(gω^j) from cpu_ref's transforms; strided and contiguous shards assemble
    to the unsharded proof"""
    import cpu_ref
    inst, (pk, _) = medium, medium_key
    cm = _cm(cc, inst)
    l, m, M = inst.l, inst.m, inst.M
    prover = cc.Prover(pk, cm)
    D = prover.domain_size
    g = 5
    vinv = pow((pow(g, D, cr.R) - 1) % cr.R, cr.R - 2, cr.R)
    try:
        for name in ("random", "max", "row0"):
            w = _witnesses(inst)[name]
            sides = []
            for k in range(2):
                v = np.zeros((D, 32), np.uint8)
                v[:m] = inst.row_values(k, w, nthreads=NT).reshape(m, 32)
                if k == 0:
                    v[m:m + l] = w.reshape(M, 32)[:l]                 # r1cs_to_qap.rs:173-177
                e = cpu_ref.ntt(cpu_ref.ntt(v, inverse=True, nthreads=NT), coset=True, nthreads=NT)
                sides.append(cr.ints_of(e))
            a = [x * vinv % cr.R for x in sides[0]]
            b = sides[1]
            assert bytes(prover.witness_map_coset_half(w, 0)) == bytes(cr.fr_bytes(a)), (name, "a side")
            assert bytes(prover.witness_map_coset_half(w, 1)) == bytes(cr.fr_bytes(b)), (name, "b side")
            assert bytes(prover.witness_map_coset(w)) == bytes(cr.fr_bytes([x * y for x, y in zip(a, b)])), name
        rng = random.Random(7)
        cases = [(inst.w, 0, 0), (inst.w, rng.randrange(cr.R), rng.randrange(cr.R)), (_witnesses(inst)["rowmax"], rng.randrange(cr.R), 0)]
        want = [prover.prove(w, r, s).data for w, r, s in cases]
        for contig in (False, True):
            shards = [cc.Prover(pk, cm, shard_rank=k, shard_count=4, contiguous_h_shards=contig) for k in range(4)]
            try:
                for (w, r, s), exp in zip(cases, want):
                    parts = b"".join(p.prove_partial(w, r) for p in shards)
                    assert shards[0].assemble(parts, 4, r, s).data == exp, contig
            finally:
                for p in shards:
                    p.close()
    finally:
        prover.close()


# ------------------------------------------------------------------------------------------- setup
def test_setup_small_equals_oracle(cc, oracle, small, small_key):
    """cg_setup on every row and column boundary == the Python oracle's key, digest for digest"""
    pk, (alpha, beta, delta, tau) = small_key
    pk_o, _ = oracle.generate_parameters(small.to_rows(), small.l, small.m, small.M, tau, alpha, beta, delta)
    g1s = lambda pts: b"".join(oracle.g1_packed(p) for p in pts)
    g2s = lambda pts: b"".join(oracle.g2_packed(p) for p in pts)
    v = pk_o["vk"]
    want = [_sha(x) for x in (g1s([v["alpha_g1"]]), g1s([pk_o["beta_g1"]]), g1s([pk_o["delta_g1"]]), g2s([v["beta_g2"]]),
                              g2s([v["gamma_g2"]]), g2s([v["delta_g2"]]), g1s(v["gamma_abc_g1"]), g1s(pk_o["a_query"]),
                              g1s(pk_o["b_g1_query"]), g2s(pk_o["b_g2_query"]), g1s(pk_o["h_query"]), g1s(pk_o["l_query"]))]
    assert _digest(pk) == want


def test_setup_medium_key_check(cc, oracle, medium, medium_key):
    """cg_setup at D = 2^17 checked by keycheck.check_key (which never goes through setup.hip)"""
    import cpu_ref
    import keycheck
    pk, trap = medium_key
    keycheck.check_key(oracle, cpu_ref, pk, _cm(cc, medium), medium.l, medium.m, medium.M, trap, nthreads=NT)


# ------------------------------------------------------------------------------------------- proofs
@pytest.mark.parametrize("coeff_basis", [False, True], ids=["folded", "coefficient_basis"])
def test_proofs_both_arrangements(cc, oracle, medium, medium_key, coeff_basis):
    """folded key (C in the l query) and the reference arrangement, staged load off and on (before and after wait_ready),
    r = s = 0 and random: every proof == cpu_ref.prove; one passes the pairing check and refuses a flipped input"""
    import cpu_ref
    import keycheck
    inst, (pk, _) = medium, medium_key
    cm = _cm(cc, inst)
    rng = random.Random(9)
    cases = [(0, 0), (rng.randrange(cr.R), rng.randrange(cr.R))]
    want = [cpu_ref.prove(pk, inst.mats, inst.l, inst.m, inst.M, inst.w, r, s, nthreads=NT) for r, s in cases]
    for staged in (False, True):
        p = cc.Prover(pk, cm, h_coefficient_basis=coeff_basis, staged_load=staged)
        try:
            rounds = ("before", "after") if staged else ("loaded",)
            for when in rounds:
                if when == "after":
                    assert p.wait_ready(300_000)
                for (r, s), exp in zip(cases, want):
                    got = p.prove(inst.w, r, s).data
                    assert got == exp, (staged, when, r == 0)
        finally:
            p.close()
    assert keycheck.verify(oracle, pk, inst.l, inst.w, got)           # the pairing check; a flipped public input is refused


def test_small_proofs_equal_cpu_ref(cc, small, small_key):
    """the small instance (rows up to 262145 terms over 300 wires): both arrangements, every witness kind"""
    import cpu_ref
    cm = _cm(cc, small)
    pk = small_key[0]
    rng = random.Random(10)
    for coeff_basis in (False, True):
        p = cc.Prover(pk, cm, h_coefficient_basis=coeff_basis)
        try:
            for name, w in _witnesses(small).items():
                r, s = rng.randrange(cr.R), rng.randrange(cr.R)
                assert p.prove(w, r, s).data == cpu_ref.prove(pk, small.mats, small.l, small.m, small.M, w, r, s, nthreads=NT), \
                    (coeff_basis, name)
        finally:
            p.close()


# ------------------------------------------------------------------------------------------- the limit
def test_row_of_exactly_8_to_the_8_terms(cc):
    """A with one row of 8^8 terms (8 sliced levels, all literal ones) proves like cpu_ref; 8^8 + 1 terms is refused at load
    (Prover and QapContext) and the process still proves afterwards"""
    import cpu_ref
    l, m, M = 2, 64, 4096
    mats, w = cr.long_row_matrix(l, m, M, cr.SELL_LIMIT + 1, seed=8)
    A = mats[0]
    # the 8^8 row: the same arrays without the row's first term (views, no copy)
    rp = A.row_ptr.copy()
    rp[1:] -= 1
    ok = (cpu_ref.Csr(rp, A.col[1:], A.coeff[32:]), mats[1], mats[2])
    assert int(rp[1]) == cr.SELL_LIMIT and int(A.row_ptr[1]) == cr.SELL_LIMIT + 1
    cm_ok = cc.ConstraintMatrices(*ok, l, M - l, m)
    cm_bad = cc.ConstraintMatrices(*mats, l, M - l, m)
    pk = cc.generate_parameters_with_qap(cm_ok, *_trap(8))
    rng = random.Random(8)
    r, s = rng.randrange(cr.R), rng.randrange(cr.R)
    want = cpu_ref.prove(pk, ok, l, m, M, w, r, s, nthreads=NT)
    p = cc.Prover(pk, cm_ok)
    try:
        assert p.prove(w, r, s).data == want
        assert bytes(p.witness_map(w)) == bytes(cpu_ref.witness_map(ok, l, m, M, w, nthreads=NT))
    finally:
        p.close()
    with pytest.raises(cc.CrescentGpuError) as ei:
        cc.Prover(pk, cm_bad)
    assert ei.value.code == -1, ei.value
    with pytest.raises(cc.CrescentGpuError):
        cc.QapContext(cm_bad)
    p = cc.Prover(pk, cm_ok)
    try:
        assert p.prove(w, r, s).data == want
    finally:
        p.close()
