"""tests/t256_steer_vectors.py against its own trace model and the oracle: every steered row hits the site it is named for - a
condition, not a statistic -, the model's final point is the oracle's for every row, every steered generator is on the curve,
no random row hits anything, and the sites no input can reach are shown not to be.  The same rows go through the host build of
csrc/t256.hpp (tests/cpp/test_t256.cpp's `row`), which takes another order of operations: bytes only.  A search that runs out
raises, so nothing is skipped.  Pure CPU."""
import os
import random
import subprocess

import pytest

import t256_steer_vectors as S
import t256_vectors as V
from conftest import ROOT

PT, Q, R = S.PT, S.Q, S.R
SRC = os.path.join(ROOT, "tests", "cpp", "test_t256.cpp")
le = lambda v: V.scalar_bytes(v).hex()


def by_words(a, b):
    """a word-by-word Montgomery product before its last conditional subtraction, as csrc/ft256.hpp runs it"""
    minv = -pow(PT, -1, 1 << 32) % (1 << 32)
    t = 0
    for i in range(8):
        t += a * ((b >> (32 * i)) & 0xffffffff)
        t += (t * minv % (1 << 32)) * PT
        assert t % (1 << 32) == 0
        t >>= 32
    return t


def test_the_model_is_the_word_by_word_product_and_the_roots_are_roots():
    rng = random.Random(0x7C01)
    pairs = [(PT - 1, PT - 1), (0, 0), (1, 1), (PT - 1, 1), (S.R2, PT - 1)] + [(rng.randrange(PT), rng.randrange(PT)) for _ in range(200)]
    for a, b in pairs:
        assert by_words(a, b) == S.pre(a, b) < 2 * PT and S.pre(a, b) % PT == a * b * pow(R, -1, PT) % PT
    assert S.rare(PT) and S.rare(R - 1) and not S.rare(PT - 1) and not S.rare(R)
    assert S.DELTA_MAX == R - 1 - PT and PT % 4 == 3 and (PT - 1) % 27 == 0 and (PT - 1) % 81 and (PT - 1) % 7 == 0 and (PT - 1) % 49
    for k in (3, 7):
        assert all(pow(S.kth_root(pow(x, k, PT), k), k, PT) == pow(x, k, PT) for x in range(2, 40))
        assert sum(S.kth_root(x, k) is not None for x in range(2, 302)) < 300 * 2 // k
    pt = S.lift_x(5, V.G[1] & 1)
    assert pt == V.G and S.lift_x(5, 1 - (V.G[1] & 1)) == V.neg(V.G)
    y = S.unmont(12345)
    while S.x_of_y(y) is None:
        y = S.unmont(S.mont(y) + 1)
    assert V.on_curve((S.x_of_y(y), y))
    # a line through three points of the curve: the cubic splits, and the least root is one of the three
    a, b = V.mul(3, V.G), V.mul(10, V.G)
    lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, PT) % PT
    third = V.neg(V.add(a, b))
    assert S.least_root([-(a[0] * b[0] * third[0]) % PT, (a[0] * b[0] + a[0] * third[0] + b[0] * third[0]) % PT, -lam * lam % PT, 1]) == min(a[0], b[0], third[0])


def test_family_counts_and_generators_on_the_curve():
    fams = S.families()
    assert [name for name, _ in S.FAMILIES] == list(fams) == list(S.COUNTS)
    for name, fam in fams.items():
        steered = [r for r in fam.rows if r.site]
        assert len(steered) == S.COUNTS[name] and len(fam.rows) == len(steered) + 2, name
        assert all(V.on_curve(p) and p is not None for p in fam.gens.points + [fam.gens.h]), name
        assert len(set(fam.gens.points)) == fam.gens.n and S.lanes_log(fam.gens.n) == 2, name      # W = 4
        assert all(len(r.z) == fam.gens.n and all(0 <= v < Q for v in r.z) and 0 <= r.blind < Q for r in fam.rows)
    names = [r.name for fam in fams.values() for r in fam.rows if r.site]
    assert len(set(names)) == len(names) == sum(S.COUNTS.values())


@pytest.mark.parametrize("name", [n for n, _ in S.FAMILIES])
def test_every_row_hits_its_site_and_the_model_ends_where_the_oracle_does(name):
    fam = S.families()[name]
    entry = S.entries(fam.gens.points, fam.gens.h)
    want = S.expected(name)
    for row, (status, out) in zip(fam.rows, want):
        point, tr = S.trace_row(entry, list(row.z), row.blind)
        assert status == V.MADE and V.compressed(point) == out, row.name
        if row.site:
            assert row.site in S.sites(tr), (row.name, tr.hits)
            assert not any(op.startswith("from_mont") for _, op, _ in tr.hits)
        else:
            assert not tr.hits, (row.name, tr.hits)
    V.assert_both_parities([out for _, out in want])
    # where the site sits, family by family
    steered = [(r, S.trace_row(entry, list(r.z), r.blind)[1]) for r in fam.rows if r.site]
    if name in ("finish_x", "finish_y"):
        assert V.parities([out for r, (_, out) in zip(fam.rows, want) if r.site]) == {0, 1}
        assert all(S.mont(p[name == "finish_y"]) < 1 << 200 for p in fam.gens.points)
    if name == "inv_last":
        assert all(("inv", "last", 511) in tr.hits for _, tr in steered)
        assert all(S.mont(pow(p[1], -7, PT)) < 1 << 200 for p in fam.gens.points)
    if name == "mixed_sum":
        sums = [S.mont(p[0]) + S.mont(p[1]) - PT for p in fam.gens.points]
        assert sums == list(S.MIXED_SUM_DELTAS) and sums[0] == 0 and sums[-1] == R - 1 - PT and len(set(sums)) >= 3
        assert all(("mixed", "q: x+y", (j, j, 0)) in tr.hits for j, (_, tr) in enumerate(steered))
    if name == "butterfly":
        assert [r.z for r, _ in steered] == [(1, 1, 0), (1, 0, 1)] and all(r.blind == 0 for r, _ in steered)
        assert ("butterfly s=1", "zz", 0) in steered[0][1].hits and ("butterfly s=2", "yy", 0) in steered[1][1].hits
        assert len(S.BUTTERFLY_TRIED) == 2
    if name == "table_entry":
        wd = [(w, d) for w, d in S.TABLE_ENTRIES]
        assert any(w >= 1 for w, _ in wd) and any(d >= 2 for _, d in wd) and (0, 1) not in wd
        for (w, d), (r, _), p in zip(wd, steered, fam.gens.points):
            assert max(r.z) == d << (8 * w) and S.mont(V.mul(d << (8 * w), p)[0]) < 1 << 200


def test_sites_that_no_input_reaches():
    """ft256_from_mont: (a + m p_T) / 2^256 < p_T for every a < p_T and every quotient m < 2^256 (t256_steer_vectors.
    from_mont_reachable has the bound).  The products of constants - to_mont(1) at the head of ft256_inv, b and 1 of t256_curve -
    have one value each, and none is in the range."""
    assert not S.from_mont_reachable()
    rng = random.Random(0x7C02)
    for a in [0, 1, PT - 1, PT - 2, S.DELTA_MAX, 1 << 255] + [rng.randrange(PT) for _ in range(500)] + [rng.randrange(1, 1 << 200) for _ in range(100)]:
        assert S.pre(a, 1) < PT and S.pre(a, 1) == S.unmont(a)
    assert S.pre(1, S.R2) == S.ONE and S.pre(V.B, S.R2) == S.CB and not S.rare(S.pre(1, S.R2)) and not S.rare(S.pre(V.B, S.R2))


def test_a_subtraction_that_is_merely_missed_is_absorbed_in_every_family():
    """A finding, not a wish.  With the subtraction LEFT OUT in the rare case the value stays in [p_T, 2^256); a product takes
    any operand below 2^256, a sum of it carries into the ninth bit and a difference borrows, so the next operation brings it
    back below p_T with the right residue, and the last operation in front of the bytes, ft256_from_mont, cannot leave such a
    value (above).  The model run that way ends on the oracle's bytes for every steered row although every row still hits its
    site: whole rows show a WRONG value in the rare case, not a missed subtraction; for that there are the single operations
    of tests/test_t256_host.py, on the host's build of the same header."""
    for name, fam in S.families().items():
        entry = S.entries(fam.gens.points, fam.gens.h)
        for row, (_, out) in zip(fam.rows, S.expected(name)):
            if row.site:
                point, tr = S.trace_row(entry, list(row.z), row.blind, missed=True)
                assert row.site in S.sites(tr) and V.compressed(point) == out and max(point) < PT, row.name
    # the difference of eight-word values as ft256_sub takes it, on operands in [p_T, 2^256) too
    assert S.Trace.sub(5, 7) == PT - 2 and S.Trace.sub(PT + 3, 3) == PT and S.Trace.sub(3, PT + 3) == 0 and S.Trace.sub(1, PT + 3) == R - 2


def random_rows():
    """2000 seeded rows of one uniform scalar and a uniform blind over one set with known logarithms, W = 2"""
    rng = random.Random(0x7C03)
    return V.make_gens(0x7C04, 1), [((rng.randrange(Q),), rng.randrange(Q)) for _ in range(2000)]


def test_no_random_row_hits_any_site():
    gens, rows = random_rows()
    entry = S.full_tables(gens.points, gens.h)
    ops = 0
    for i, (z, blind) in enumerate(rows):
        point, tr = S.trace_row(entry, list(z), blind)
        assert not tr.hits, (i, tr.hits)
        ops += tr.ops
        if i < 12:
            assert V.compressed(point) == gens.commit(list(z), blind)[1], i
    assert ops > 2000 * 1500                              # some three million sums and products, none in the rare case


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("t256steer") / "test_t256")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", path, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def test_the_host_build_writes_the_same_bytes(exe):
    lines, want, names = [], [], []
    for name, fam in S.families().items():
        for row, (status, out) in zip(fam.rows, S.expected(name)):
            lines.append("row %d %s %s %s %s" % (fam.gens.n, fam.gens.g_xy.hex(), fam.gens.h_xy.hex(), "".join(le(v) for v in row.z), le(row.blind)))
            want.append("%d%s" % (status, out.hex()))
            names.append(row.name)
    gens, rows = random_rows()
    for z, blind in rows[:12]:
        lines.append("row 1 %s %s %s %s" % (gens.g_xy.hex(), gens.h_xy.hex(), le(z[0]), le(blind)))
        status, out = gens.commit(list(z), blind)
        want.append("%d%s" % (status, out.hex()))
        names.append("random")
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = r.stdout.split()
    assert len(got) == len(lines) == sum(S.COUNTS.values()) + 2 * len(S.COUNTS) + 12
    for g, w, n in zip(got, want, names):
        assert g == w, n
