"""cg_poseidon_p256_permute_batch and cg_hq_batch (csrc/devicelinkmake.hip; csrc/poseidon_p256.hpp, csrc/fp256.hpp) on the
inputs of tests/steer_vectors.py.  Each state takes one add or product site of the permutation's first round into the rare
branch of `f256_reduce_once` - no ninth bit, yet not below p -, which pseudo-random states meet about once in 2^32 operations;
the round loop is rolled on the device, so the first round's instructions are every round's.  Each h_Q triple does the same to
the conversion of q0 or q1, or to the sum in front of the second permutation.  tests/test_steer_vectors_cpu.py shows that every
input hits its site, and that six of the matrix's nine products cannot take the branch at all.

Expected bytes are tests/poseidon_vectors.py's, computed once per module; every comparison is byte for byte."""
import random

import pytest

import poseidon_vectors as PV
import steer_vectors as S
import test_gpu_device_link_make as M

pytestmark = pytest.mark.gpu

P, FR = S.P, S.FR
MADE = 1
FAMILIES = [name for name, _ in S.POSEIDON_FAMILIES]
fe = lambda v: int(v).to_bytes(32, "little")
triple = lambda q: b"".join(fe(x) for x in q)


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


@pytest.fixture(scope="module")
def world(cc):
    w = M.World(cc, "mdl", 0x905E)
    yield w
    w.pvk.close()


@pytest.fixture(scope="module")
def oracle():
    """family -> [(name, state, permuted)], the same for 44 random states under "random"; and [(name, triple, h_Q)] for the
    steered triples and for 60 random ones"""
    c = PV.p256()
    rng = random.Random(0x905E0)
    perm = lambda name, st: (name, tuple(st), triple(PV.permute(c, list(st))))
    states = {name: [perm(v.name, v.state) for v in vecs] for name, vecs in S.poseidon_families().items()}
    states["random"] = [perm("random %d" % i, [rng.randrange(P) for _ in range(3)]) for i in range(44)]
    hq = lambda name, q: (name, tuple(q), PV.hq(*q))
    triples = {"steered": [hq(v.name, v.q) for v in S.hq_vectors()],
               "random": [hq("random %d" % i, [rng.randrange(FR) for _ in range(3)]) for i in range(60)]}
    return states, triples


def run_permute(world, rows):
    assert 0 < len(rows) < 200
    out, status = world.cc.Groth16.poseidon_p256_permute_batch_packed(world.pvk, b"".join(triple(st) for _, st, _ in rows))
    assert status.tolist() == [MADE] * len(rows)
    for i, (name, _, want) in enumerate(rows):
        assert out[i].tobytes() == want, (i, name)


def run_hq(world, rows):
    assert 0 < len(rows) < 200
    h, status = world.cc.Groth16.hq_batch_packed(world.pvk, b"".join(triple(q) for _, q, _ in rows))
    assert status.tolist() == [MADE] * len(rows)
    for i, (name, _, want) in enumerate(rows):
        assert h[i].tobytes() == want, (i, name)


@pytest.mark.parametrize("family", FAMILIES)
def test_a_family_of_states_in_one_batch_between_random_states(world, oracle, family):
    states, _ = oracle
    assert len(states[family]) == S.POSEIDON_COUNTS[family]
    run_permute(world, states["random"][:2] + states[family] + states["random"][2:4])


def test_steered_triples_in_one_batch_between_random_triples(world, oracle):
    _, triples = oracle
    assert len(triples["steered"]) == S.POSEIDON_COUNTS["hq"]
    run_hq(world, triples["random"][:2] + triples["steered"] + triples["random"][2:4])


def test_all_families_interleaved_with_random_rows(world, oracle):
    states, triples = oracle
    lists = [list(states[f]) for f in FAMILIES]
    merged = []
    while any(lists):                                                   # round robin over the families
        merged += [rows.pop(0) for rows in lists if rows]
    batch = [row for pair in zip(merged, states["random"]) for row in pair] + states["random"][len(merged):]
    assert len(merged) == 27 and 65 <= len(batch) < 200 and set(merged) <= set(batch)
    run_permute(world, batch)
    batch = list(triples["random"])
    for i, row in enumerate(triples["steered"]):
        batch.insert(5 + 11 * i, row)
    assert 65 <= len(batch) < 200
    run_hq(world, batch)
