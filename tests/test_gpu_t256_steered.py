"""cg_t256_commit_rows_batch (csrc/t256commit.hip; csrc/t256.hpp, csrc/ft256.hpp) on the generator sets and rows of
tests/t256_steer_vectors.py: rows that take the rare case of `ft256_reduce_once` - no ninth bit, yet not below p_T - in the
last products of k_t256_finish, in the last step of `ft256_inv`, in the sum q.x + q.y of `t256_add_mixed` on a table entry, and
in the products `zz` and `yy` of `t256_add` inside the LDS butterfly.  Pseudo-random rows meet that case about once in 2^32
operations, so without these rows the gfx950 code of it never runs.  tests/test_t256_steer_cpu.py shows, with a trace model
of the device's order of operations, that every row hits its site.  What these rows show is that the gfx950 code of the case
runs and subtracts the right thing: a wrong value there changes their bytes, a subtraction merely left out does not - the next
operation absorbs it (DESIGN.md has both mutations).

Expected bytes and statuses are tests/t256_vectors.py's (the sum term by term: these generators have no known logarithm);
every comparison is byte for byte, and the outputs are filled with 0xA5 beforehand.  Each family is one handle and one call:
its steered rows beside two unsteered ones, four lanes a row."""
import pytest

import t256_steer_vectors as S
import t256_vectors as V
from test_gpu_t256_commit import call_rows, pack

pytestmark = pytest.mark.gpu

FAMILIES = [name for name, _ in S.FAMILIES]


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


@pytest.fixture(scope="module")
def handles(cc):
    """family name -> the library's handle on the family's generators, loaded once"""
    made = {}

    def get(name):
        if name not in made:
            gens = S.families()[name].gens
            made[name] = cc.T256Gens(gens.g_xy, gens.h_xy)
        return made[name]
    yield get
    for h in made.values():
        h.close()


def run(cc, handle, rows, want):
    """one call on the rows (name, z, blind), every row against the oracle's (status, bytes); the call ran four lanes a row"""
    out, status = call_rows(cc, handle, pack([v for _, z, _ in rows for v in z]), pack([b for _, _, b in rows]), len(rows))
    for i, ((name, _, _), (st, row)) in enumerate(zip(rows, want)):
        assert status[i] == st == V.MADE and out[i].tobytes() == row, (i, name, out[i].tobytes().hex(), row.hex())
    assert handle.commit_last_kernel_ms()[2] == 4


@pytest.mark.parametrize("family", FAMILIES)
def test_a_family_beside_two_unsteered_rows(cc, handles, family):
    fam, want = S.families()[family], S.expected(family)
    assert sum(r.site is not None for r in fam.rows) == S.COUNTS[family] == len(fam.rows) - 2
    V.assert_both_parities([row for _, row in want])
    run(cc, handles(family), [(r.name, r.z, r.blind) for r in fam.rows], want)


@pytest.mark.parametrize("family", ["finish_x", "finish_y", "inv_last"])
def test_the_finish_families_inside_seventy_rows(cc, handles, family):
    """70 rows at four lanes a row are four whole waves of sixteen rows and six rows of a fifth, whose other lanes are dead
    rows.  The steered rows stand at 5 and 37, neither the first row of its wave, and at 67 in the last wave; the other rows
    cycle through the family's unsteered ones."""
    fam, want = S.families()[family], S.expected(family)
    steered = [i for i, r in enumerate(fam.rows) if r.site]
    plain = [i for i, r in enumerate(fam.rows) if not r.site]
    at = {5: steered[0], 37: steered[1], 67: steered[0]}
    which = [at.get(i, plain[i % len(plain)]) for i in range(70)]
    assert all(i % 16 for i in at) and 67 // 16 == 4 == 69 // 16
    V.assert_both_parities([want[w][1] for w in which])
    run(cc, handles(family), [(fam.rows[w].name, fam.rows[w].z, fam.rows[w].blind) for w in which], [want[w] for w in which])
