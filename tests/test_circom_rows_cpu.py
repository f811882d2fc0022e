"""The circom-shaped instances of tests/circom_rows.py, and the C restatement on them (pure CPU).

The generator is checked to make what the GPU tests rely on (every row-length and column-length boundary present, hot and
repeated wires, the coefficient mix, a satisfied system), and oracle/cpu_ref.c's witness map is pinned to the Python
oracle on long repeated rows, so that it can stand as the reference at sizes the Python oracle cannot reach."""
import numpy as np
import pytest

import circom_rows as cr


@pytest.fixture(scope="module")
def ref():
    import cpu_ref
    cpu_ref.lib()
    return cpu_ref


def _row_terms(mat, i):
    lo, hi = int(mat.row_ptr[i]), int(mat.row_ptr[i + 1])
    return mat.col[lo:hi], mat.coeff.reshape(-1, 32)[lo:hi]


def _satisfied(ref, inst, w):
    """<A_i,w>·<B_i,w> == <C_i,w> for every row, each row by cpu_ref's inner product (not by the spmv the generator solves with)"""
    vals = []
    for mat in inst.mats:
        v = []
        for i in range(inst.m):
            cols, cf = _row_terms(mat, i)
            v.append(ref.fr_inner(cf, w.reshape(-1, 32)[cols]) if cols.size else 0)
        vals.append(v)
    return all(a * b % cr.R == c for a, b, c in zip(*vals))


def test_generator_shapes_and_satisfaction(ref):
    inst = cr.circom_instance(4, 200, 300, seed=11)
    R1 = cr.fr_bytes([cr.R - 1])[0]
    for k in range(3):
        lengths = inst.row_lengths(k)
        for n in cr.ROW_BOUNDARIES:
            assert lengths[inst.rows["len%d" % n]] == n, (k, n)
        counts = inst.column_counts(k)
        assert counts[inst.wires["exact4096"]] == 4096 and counts[inst.wires["exact4097"]] == 4097, k
        for hot in ("one", "hot1", "hot2"):
            assert counts[inst.wires[hot]] > 4096, (k, hot)
        mat = inst.mats[k]
        cf = mat.coeff.reshape(-1, 32)
        ones = (cf[:, 0] == 1) & ~cf[:, 1:].any(axis=1)
        assert ones.sum() > mat.nnz // 3 and (~cf.any(axis=1)).sum() > 0 and (cf == R1).all(axis=1).any(), k
        for e in (1, 64, 200, 253):
            p = np.zeros(32, np.uint8)
            p[e // 8] = 1 << (e % 8)
            assert (cf == p).all(axis=1).any(), (k, e)
        # one wire repeated with the literal one; pairs c, r - c on one wire that cancel
        cols, cfs = _row_terms(mat, inst.rows["repeat"])
        body = slice(0, 700)
        assert (cols[body] == inst.wires["hot1"]).all() and (cfs[body, 0] == 1).all() and not cfs[body, 1:].any()
        cols, cfs = _row_terms(mat, inst.rows["cancel"])
        pairs = cr.ints_of(cfs[:600])
        assert (cols[:600] == inst.wires["hot1"]).all() and all((a + b) == cr.R for a, b in zip(pairs[::2], pairs[1::2]))
    assert _satisfied(ref, inst, inst.w)
    w = inst.w.copy()
    w[32 * 7] ^= 1
    assert not _satisfied(ref, inst, w)


def test_generator_dictionary_beyond_2_to_the_20():
    inst = cr.circom_instance(20, 131_000, 133_000, seed=12, hot_terms=20_000,
                              mixes=(cr.MIX_DICT_HEAVY, cr.MIX_CIRCOM, cr.MIX_CIRCOM), dict_size=(None, 4096, 4096))
    assert len(np.unique(inst.mats[0].coeff.reshape(-1, 32), axis=0)) > 1 << 20
    for k in range(3):
        rows_with_one = np.unique(np.searchsorted(inst.mats[k].row_ptr.astype(np.int64), np.flatnonzero(inst.mats[k].col == 0),
                                                  side="right"))
        assert rows_with_one.size > 4096, k                  # wire 0 in more than 4096 constraints of every matrix
    a, b, c = (cr.ints_of(inst.row_values(k)) for k in range(3))
    assert all(x * y % cr.R == z for x, y, z in zip(a, b, c))


def test_extreme_witnesses(ref):
    inst = cr.circom_instance(4, 200, 300, seed=11)
    big = inst.rows["len262145"]
    for k, target in ((0, 0), (1, cr.R - 1), (2, cr.R - 1)):
        w = cr.extreme_witness(inst, "row", np.random.default_rng(k), (k, big), target)
        assert cr.ints_of(inst.row_values(k, w)[32 * big:32 * big + 32]) == [target]
    for kind, v in (("zeros", 0), ("max", cr.R - 1)):
        w = cr.ints_of(cr.extreme_witness(inst, kind))
        assert w[0] == 1 and set(w[1:]) == {v}


@pytest.mark.parametrize("seed", [1, 2])
def test_cpu_ref_witness_map_on_long_repeated_rows(ref, oracle, seed):
    """cpu_ref.witness_map == the Python oracle on 64 constraints with rows up to 4097 terms over 300 wires (a hot wire
    repeated, cancelling pairs, r - 1 and power-of-two coefficients), satisfying and extreme witnesses"""
    inst = cr.circom_instance(3, 64, 300, seed=seed, boundaries=(0, 1, 8, 9, 64, 65, 512, 513, 4096, 4097), exact_columns=(),
                              hot_terms=800, repeat_len=300, cancel_pairs=100)
    rows = inst.to_rows()
    ws = [inst.w, cr.extreme_witness(inst, "max"), cr.extreme_witness(inst, "row", None, (0, inst.rows["len4097"]), 0),
          cr.extreme_witness(inst, "row", None, (2, inst.rows["len4096"]), cr.R - 1)]
    for i, w in enumerate(ws):
        want = oracle.witness_map_from_matrices(rows, inst.l, inst.m, cr.ints_of(w))
        assert cr.ints_of(ref.witness_map(inst.mats, inst.l, inst.m, inst.M, w, nthreads=4)) == want, i
