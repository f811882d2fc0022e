"""The load-time key fold (csrc/ecntt.hip, sum_xyzz_by_key) on keys that hit its rare branches.  Needs an MI355X.

By default a Prover does not prove on the key as loaded: two inverse DFTs over G1 points move the h query into the coset's
evaluation basis and fold the C matrix into the l query (msm.hpp, identities (1) and (2)).  With a key made from a random
trapdoor every butterfly of k_ec_stage adds two unrelated finite points, except for the one missing last point.  The keys here
are given by discrete logarithms (tests/degenerate_keys.py) so that the butterflies, the per-wire sums of the C terms and
k_ec_fold_l meet the identity, the same point twice and a point with its negative; which key reaches which branch is counted
on the CPU by tests/test_degenerate_keys_cpu.py, and nothing is claimed here that is not asserted there.

Every comparison is of the 256 proof bytes with the proof in closed form over Python integers, which shares no DFT, MSM or fold
with the library.  Every key is loaded folded (the default) and with h_coefficient_basis=True (the key as loaded); the folded
handle proves everything twice.  The representation-dependent bounds inside the rare branches (a loaded record with X near
13 N entering dbl29, say) cannot be steered from a key: tools/bounds29.py and tests/cpp/test_field29.cpp cover those."""
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

import degenerate_keys as dk

pytestmark = pytest.mark.gpu

R = dk.R


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


CASES = dk.CASES
LOADER_CASES = ["constant/fold", "index0", "aimed_l"]


class _Case:
    """the circuit, the key by logarithms and as points, four jobs (random non-zero and all-ones witnesses, (r, s) = (0, 0) and
    a random pair) and their proofs in closed form"""

    def __init__(self, cc, name):
        self.circ, self.key, self.roles = circ, key, _ = dk.case_key(name)
        self.pk = dk.gpu_key(cc, key)
        self.cm = circ.matrices(cc)
        rng = random.Random(len(name) + circ.D)
        rs = [(0, 0), (rng.randrange(1, R), rng.randrange(1, R))]
        self.jobs = [(wn, dk.scalars(w), r, s) for wn, w in circ.witnesses().items() for r, s in rs]
        self.want = [dk.closed_form_proof(key, circ.mats, circ.m, w, r, s) for w in circ.witnesses().values() for r, s in rs]

    def mismatches(self, prove, what):
        """the jobs whose proof is not the closed form's bytes (all of them are tried, so that a failure names every one)"""
        return [(what, wn, "r = s = 0" if r == 0 else "random r, s") for (wn, w, r, s), want in zip(self.jobs, self.want)
                if prove(w, r, s) != want]


_cases = {}


def _case(cc, name):
    if name not in _cases:
        _cases[name] = _Case(cc, name)
    return _cases[name]


def test_gpu_made_points_are_the_oracles(cc):
    """the keys below are made by cc.fixed_base_g1 / g2; the same key made point by point on the CPU has the same bytes"""
    c = _case(cc, "aimed_l")
    ref = dk.proving_key_from_points(cc, dk.oracle_key(c.key))
    for f in ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query", "beta_g1", "delta_g1"):
        assert bytes(getattr(c.pk, f)) == bytes(getattr(ref, f)), f
    assert bytes(c.pk.vk.alpha_g1) == bytes(ref.vk.alpha_g1) and bytes(c.pk.vk.delta_g2) == bytes(ref.vk.delta_g2)
    lq = c.pk.l_query.reshape(-1, 64)
    assert not lq[c.roles["l_identity"] - c.circ.l].any() and lq[c.roles["doubling"] - c.circ.l].any()


@pytest.mark.parametrize("name", list(CASES))
def test_folded_and_unfolded_loads_prove_the_closed_form(cc, name):
    c = _case(cc, name)
    folded = cc.Prover(c.pk, c.cm)
    try:
        assert folded.domain_size == c.circ.D
        bad = c.mismatches(lambda w, r, s: folded.prove(w, r, s).data, "folded")
        bad += c.mismatches(lambda w, r, s: folded.prove(w, r, s).data, "folded, second prove")
    finally:
        folded.close()
    plain = cc.Prover(c.pk, c.cm, h_coefficient_basis=True)
    try:
        bad += c.mismatches(lambda w, r, s: plain.prove(w, r, s).data, "h_coefficient_basis")
    finally:
        plain.close()
    assert not bad, bad


@pytest.mark.parametrize("name", LOADER_CASES)
def test_staged_load(cc, name):
    """the warm-up arrangement and, after the worker thread has folded the key, the final one"""
    c = _case(cc, name)
    p = cc.Prover(c.pk, c.cm, staged_load=True)
    try:
        bad = c.mismatches(lambda w, r, s: p.prove(w, r, s).data, "before wait_ready")
        assert p.wait_ready(120_000)
        bad += c.mismatches(lambda w, r, s: p.prove(w, r, s).data, "after wait_ready")
        assert not bad, bad
    finally:
        p.close()


@pytest.mark.parametrize("split", ["strided", "contiguous", "span"])
@pytest.mark.parametrize("name", LOADER_CASES)
def test_two_shards_assemble_to_the_closed_form(cc, name, split):
    """each shard folds the whole key and keeps its part of the two tables: the coset points j = rank (mod 2), halves, or
    30 % and 70 % of every query"""
    c = _case(cc, name)
    kw = {"strided": [{}, {}], "contiguous": [dict(contiguous_h_shards=True)] * 2,
          "span": [dict(shard_span=(0, 3000)), dict(shard_span=(3000, 10000))]}[split]
    shards = []
    try:
        for k in range(2):
            shards.append(cc.Prover(c.pk, c.cm, shard_rank=k, shard_count=2, **kw[k]))
        bad = c.mismatches(lambda w, r, s: shards[0].assemble(b"".join(p.prove_partial(w, r) for p in shards), 2, r, s).data, split)
        assert not bad, bad
    finally:
        for p in shards:
            p.close()


@pytest.mark.parametrize("name", LOADER_CASES)
def test_three_slots_throughput(cc, name):
    c = _case(cc, name)
    p = cc.Prover(c.pk, c.cm, proof_slots=3, mode="throughput")
    try:
        assert p.info()["proof_slots"] == 3
        for rnd in range(2):
            with ThreadPoolExecutor(max_workers=3) as ex:
                got = list(ex.map(lambda j: p.prove(j[1], j[2], j[3]).data, c.jobs))
            for (wn, _, r, _), g, want in zip(c.jobs, got, c.want):
                assert g == want, (wn, r == 0, "round %d" % rnd)
    finally:
        p.close()
