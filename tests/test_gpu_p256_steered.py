"""cg_p256_tu_batch and cg_p256_rtu_batch (csrc/p256tu.hip; csrc/p256.hpp, csrc/fq256.hpp, csrc/fp256.hpp) on the rows of
tests/steer_vectors.py: R.x in [n, p), digests that are 0 mod n or not below n, scalars with structure in the table walk and
in the windowed chain, and coordinates and scalars that take the rare branch of `f256_reduce_once` / `q256_reduce_once` - no
ninth bit, yet not below the modulus - at the fields' entry points.  Pseudo-random rows meet that branch about once in 2^32
operations, so without these rows the gfx950 code of it never runs.  tests/test_steer_vectors_cpu.py shows that every row hits
its case.

Expected bytes and statuses are tests/p256_vectors.py's, computed once per module; every comparison is byte for byte.  Each
family is one batch per entry with two honest rows at either end, and all families go once more through one batch per entry
with honest rows in between, so that steered rows share waves with ordinary ones."""
import pytest

import p256_vectors as V
import steer_vectors as S
import test_gpu_device_link_make as M

pytestmark = pytest.mark.gpu

FAMILIES = [name for name, _ in S.P256_FAMILIES]


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


@pytest.fixture(scope="module")
def world(cc):
    w = M.World(cc, "mdl", 0x57E0)
    yield w
    w.pvk.close()


@pytest.fixture(scope="module")
def oracle():
    """(steered, honest): family -> kind -> [(name, args, want)], and kind -> the same for 36 honest rows; want is
    (status, t, u) for "tu" and (status, r, t, u) for "rtu" """
    steered = {name: {kind: [(v.name, v.args, S.expected(v)) for v in vecs if v.kind == kind] for kind in ("tu", "rtu")}
               for name, vecs in S.p256_families().items()}
    honest = {"tu": [], "rtu": []}
    for i, row in enumerate(V.signed_rows(0x57E1, 36)):
        st, r, t, u = V.compute_rtu(*row)
        assert st == V.MADE
        honest["rtu"].append(("honest %d" % i, row, (st, r, t, u)))
        honest["tu"].append(("honest %d" % i, (r, row[2]), (st, t, u)))
    return steered, honest


def run(world, kind, rows):
    """one call of the entry on the rows' arguments, every row against the oracle"""
    assert 0 < len(rows) < 200
    call = world.cc.Groth16.p256_tu_batch if kind == "tu" else world.cc.Groth16.p256_rtu_batch
    n_args = 2 if kind == "tu" else 3
    *outs, status = call(world.pvk, *[b"".join(args[j] for _, args, _ in rows) for j in range(n_args)])
    assert len(status) == len(rows)
    for i, (name, _, want) in enumerate(rows):
        assert (int(status[i]),) + tuple(o[i].tobytes() for o in outs) == want, (i, name)


@pytest.mark.parametrize("family", FAMILIES)
def test_a_family_in_one_batch_between_honest_rows(world, oracle, family):
    steered, honest = oracle
    for kind in ("tu", "rtu"):
        rows = steered[family][kind]
        assert rows
        run(world, kind, honest[kind][:2] + rows + honest[kind][2:4])
    assert sum(len(steered[family][kind]) for kind in ("tu", "rtu")) == S.P256_COUNTS[family]


def test_all_families_interleaved_with_honest_rows(world, oracle):
    steered, honest = oracle
    for kind, every in (("tu", 1), ("rtu", 3)):
        lists = [list(steered[f][kind]) for f in FAMILIES]
        merged = []
        while any(lists):                                               # round robin over the families
            merged += [rows.pop(0) for rows in lists if rows]
        spare = list(honest[kind])
        batch = []
        for i, row in enumerate(merged):
            batch.append(row)
            if i % every == every - 1 and spare:
                batch.append(spare.pop(0))
        assert 65 <= len(batch) < 200 and len(merged) == sum(len(steered[f][kind]) for f in FAMILIES) and len(batch) - len(merged) >= 29
        assert {want[0] for _, _, want in batch} == ({V.MADE} if kind == "tu" else {V.MADE, V.MALFORMED, V.BAD_SIGNATURE})
        run(world, kind, batch)
