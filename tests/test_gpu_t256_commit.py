"""pi2's witness commitment on the GPU (csrc/t256commit.hip: cg_t256_gens_load, cg_t256_commit_rows_batch,
cg_hyrax_commit_batch; csrc/t256.hpp, csrc/ft256.hpp): Pedersen vector commitments in T-256 over one set of generators, and
the Hyrax commitment of a batch of proofs on them.

Expected bytes and statuses come from tests/t256_vectors.py, a pure-Python restatement over integers that shares no code with
the library (tests/test_t256_cpu.py holds it against itself).  Generators are known multiples of G, so a row's expected value
is ONE scalar multiplication whatever its width.  Every comparison is byte for byte, statuses included; every test asserts
that both values of the parity bit occur among its expected outputs.  The calls go through the C ABI with the outputs filled
with 0xA5 beforehand, so that a byte the library should have written and did not shows."""
import ctypes
import os
import random

import numpy as np
import pytest

import t256_vectors as V
from conftest import ROOT

pytestmark = pytest.mark.gpu

Q = V.Q
MADE, MALFORMED = V.MADE, V.MALFORMED
FILL = 0xA5


CHUNK_ROWS = 1 << 14        # csrc/t256commit.hip's T256_CHUNK_ROWS: the rows of one launch set


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


class Sets:
    """generator sets by width, each made once: the oracle's Gens and the library's handle"""

    def __init__(self, cc):
        self.cc, self.made = cc, {}

    def __call__(self, n):
        if n not in self.made:
            self.add(n, V.make_gens(0x6E00 + n, n))
        return self.made[n]

    def add(self, key, gens):
        self.made[key] = (gens, self.cc.T256Gens(gens.g_xy, gens.h_xy))
        return self.made[key]

    def close(self):
        for _, h in self.made.values():
            h.close()


@pytest.fixture(scope="module")
def sets(cc):
    s = Sets(cc)
    yield s
    s.close()


def pack(values):
    return np.frombuffer(b"".join(V.scalar_bytes(v) for v in values), np.uint8).copy()


def call_rows(cc, handle, scalars, blinds, n):
    out, status = np.full((n, 33), FILL, np.uint8), np.full(n, FILL, np.uint8)
    rc = cc.lib().cg_t256_commit_rows_batch(handle._h, scalars.ctypes.data, blinds.ctypes.data, n, out.ctypes.data, status.ctypes.data)
    assert rc == 0, cc.lib().cg_last_error()
    return out, status


def call_hyrax(cc, handle, num_vars, vars_, blinds, n):
    L = V.factored_lens(num_vars)[0]
    out, status = np.full((n, L, 33), FILL, np.uint8), np.full(n, FILL, np.uint8)
    rc = cc.lib().cg_hyrax_commit_batch(handle._h, num_vars, vars_.ctypes.data, blinds.ctypes.data, n, out.ctypes.data, status.ctypes.data)
    assert rc == 0, cc.lib().cg_last_error()
    return out, status


def check_rows(cc, gens, handle, rows):
    """rows of (z, blind) through the rows call against the oracle, row by row; returns the expected (status, bytes)"""
    want = [gens.commit(z, b) for z, b in rows]
    out, status = call_rows(cc, handle, pack([v for z, _ in rows for v in z]), pack([b for _, b in rows]), len(rows))
    for i, (st, row) in enumerate(want):
        assert status[i] == st and out[i].tobytes() == row, (i, status[i], out[i].tobytes().hex(), row.hex())
    return want


# ---- the rows call at every width the kernel treats differently ---------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 64, 128])
def test_rows_call_byte_for_byte(cc, sets, n):
    """n_gens = 1 is Scalar::commit (two lanes a row, 32 rows a wave: a lane has sixteen windows of either term), 4 is below
    a wave (eight lanes a row, four windows of every term a lane), 64 and 128 are a whole wave a row: a lane has one window
    of every other term"""
    gens, handle = sets(n)
    assert handle.n_gens == n and handle.table_bytes == (n + 1) * 32 * 255 * 64
    rng = random.Random(0x5000 + n)
    rows = [([rng.randrange(Q) for _ in range(n)], rng.randrange(Q)) for _ in range(3)]
    rows += [(V.mixed_scalars(rng, n), rng.randrange(Q)) for _ in range(3)]
    rows += [([0] * n, rng.randrange(1, Q)), ([rng.randrange(Q)] + [0] * (n - 1), 0)]
    want = check_rows(cc, gens, handle, rows)
    assert all(st == MADE for st, _ in want)
    V.assert_both_parities([r for _, r in want])
    assert handle.commit_last_kernel_ms()[2] == min(64, 1 << n.bit_length())


# ---- Hyrax ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_vars", [2, 3, 7, 13])
def test_hyrax_two_proofs_and_the_rows_call_on_the_same_data(cc, sets, num_vars):
    """2 x 2, 2 x 4 (odd: L != R), 8 x 16 and 64 x 128; the rows call on the same arrays writes the same bytes"""
    L, R = V.factored_lens(num_vars)
    gens, handle = sets(R)
    rng = random.Random(0x4A00 + num_vars)
    proofs = [([rng.randrange(Q) for _ in range(L * R)], [rng.randrange(Q) for _ in range(L)]),
              (V.mixed_scalars(rng, L * R), [rng.randrange(Q) for _ in range(L)])]
    want = [V.hyrax(gens, num_vars, v, b) for v, b in proofs]
    vars_, blinds = pack([x for v, _ in proofs for x in v]), pack([x for _, b in proofs for x in b])
    out, status = call_hyrax(cc, handle, num_vars, vars_, blinds, 2)
    for i, (st, rows) in enumerate(want):
        assert st == MADE and status[i] == st and out[i].tobytes() == rows, i
    V.assert_both_parities([out[i, j].tobytes() for i in range(2) for j in range(L)])
    out_rows, status_rows = call_rows(cc, handle, vars_, blinds, 2 * L)
    assert out_rows.tobytes() == out.tobytes() and (status_rows == MADE).all()
    # the Python wrapper returns the same
    out_py, status_py = handle.hyrax_commit_batch(num_vars, vars_, blinds)
    assert out_py.tobytes() == out.tobytes() and status_py.tolist() == [MADE, MADE]


def test_hyrax_refuses_a_set_of_the_wrong_width(cc, sets):
    _, handle = sets(4)
    buf = np.full(4096, FILL, np.uint8)
    p = buf.ctypes.data
    for num_vars in (2, 5, 6, 64):
        assert cc.lib().cg_hyrax_commit_batch(handle._h, num_vars, p, p, 1, p, p) == -1 and b"generators" in cc.lib().cg_last_error()
    assert cc.lib().cg_hyrax_commit_batch(handle._h, 3, None, p, 1, p, p) == -1 and b"null" in cc.lib().cg_last_error()
    assert cc.lib().cg_t256_commit_rows_batch(handle._h, p, p, 1, None, p) == -1 and b"null" in cc.lib().cg_last_error()
    assert (buf == FILL).all()


# ---- rows steered to what random rows miss -----------------------------------------------------------------------------------------
def test_steered_rows(cc, sets):
    gens, handle = sets(4)
    rng = random.Random(0x57EE8)
    z = [rng.randrange(Q) for _ in range(4)]
    cancel = -gens.row_scalar(z, 0) * pow(gens.kh, -1, Q) % Q                   # the blind that cancels the vector part
    rows = [([0, 0, 0, 0], 0), (z, cancel), ([1, Q - 1, V.TOP_DIGIT, 1], 1), ([Q - 1] * 4, Q - 1), ([V.TOP_DIGIT] * 4, V.TOP_DIGIT),
            ([1, 1, 1, 1], 0), (z, 7)]
    want = check_rows(cc, gens, handle, rows)
    assert want[0] == (MADE, V.IDENTITY_COMPRESSED) and want[1] == (MADE, V.IDENTITY_COMPRESSED)
    V.assert_both_parities([r for _, r in want])


def test_partials_that_cancel_and_coincide_inside_the_butterfly(cc, sets):
    """Two generators and the blind over four lanes.  Of the rows ([1, 1], 0) the digit of g_0 falls to lane 0 and that of g_1
    to lane 1, which meet in the butterfly's last step as P + (-P) or as P + P; the wider rows spread both scalars over all
    four lanes, and the last step's two halves still cancel where the row's sum is the identity"""
    rng = random.Random(0xB077E)
    k0, kh = rng.randrange(1, Q), rng.randrange(1, Q)
    all_want = []
    for key, ks in (("opposite", [k0, Q - k0]), ("equal", [k0, k0])):
        gens, handle = sets.add(key, V.Gens(ks, kh))
        s = rng.randrange(1, Q)
        rows = [([s, s], 0), ([s, s], rng.randrange(1, Q)), ([s, Q - s], 0), ([1, 1], 0), ([s, rng.randrange(Q)], rng.randrange(Q))]
        want = check_rows(cc, gens, handle, rows)
        # g_1 = -g_0 with equal scalars and no blind: P + (-P) in the last step, the identity's bytes; g_1 = g_0: P + P
        assert (want[0][1] == V.IDENTITY_COMPRESSED) == (key == "opposite")
        assert (want[2][1] == V.IDENTITY_COMPRESSED) == (key == "equal")
        all_want += want
    V.assert_both_parities([r for _, r in all_want])


def test_a_malformed_row_is_that_row_only(cc, sets):
    gens, handle = sets(4)
    rng = random.Random(0xBAD)
    good = lambda: ([rng.randrange(Q) for _ in range(4)], rng.randrange(Q))
    rows = [good(), ([1, Q, 1, 1], 5), good(), ([1, 1, 1, (1 << 256) - 1], 5), good(), ([1, 1, 1, 1], Q), ([Q - 1] * 4, Q - 1), good()]
    want = check_rows(cc, gens, handle, rows)
    assert [st for st, _ in want] == [MADE, MALFORMED, MADE, MALFORMED, MADE, MALFORMED, MADE, MADE]
    assert all(r == V.ZERO_ROW for st, r in want if st == MALFORMED)
    V.assert_both_parities([r for _, r in want])


def test_a_malformed_scalar_takes_its_whole_proof_and_no_neighbour(cc, sets):
    num_vars = 3
    L, R = V.factored_lens(num_vars)
    gens, handle = sets(R)
    rng = random.Random(0xBAD2)
    proofs = [([rng.randrange(Q) for _ in range(L * R)], [rng.randrange(Q) for _ in range(L)]) for _ in range(4)]
    proofs[1][0][L * R - 1] = Q                                                 # the last scalar of the last row
    proofs[3][1][0] = (1 << 256) - 1                                            # a blind
    want = [V.hyrax(gens, num_vars, v, b) for v, b in proofs]
    assert [st for st, _ in want] == [MADE, MALFORMED, MADE, MALFORMED]
    out, status = call_hyrax(cc, handle, num_vars, pack([x for v, _ in proofs for x in v]), pack([x for _, b in proofs for x in b]), 4)
    for i, (st, rows) in enumerate(want):
        assert status[i] == st and out[i].tobytes() == rows, i
    assert want[1][1] == V.ZERO_ROW * L
    V.assert_both_parities([out[i, j].tobytes() for i in (0, 2) for j in range(L)])


# ---- chunks and the choice of lanes per row -----------------------------------------------------------------------------------------
def cycled(gens, rows, count):
    """`count` rows that cycle through the distinct `rows`: the arrays, and what the oracle makes of the distinct ones"""
    want = [gens.commit(z, b) for z, b in rows]
    reps = -(-count // len(rows))
    scal = np.tile(pack([v for z, _ in rows for v in z]), reps)[:32 * gens.n * count].copy()
    blind = np.tile(pack([b for _, b in rows]), reps)[:32 * count].copy()
    want_out = np.tile(np.frombuffer(b"".join(r for _, r in want), np.uint8), reps)[:33 * count]
    want_status = np.tile(np.array([st for st, _ in want], np.uint8), reps)[:count]
    return scal, blind, want_out, want_status, want


def test_a_call_that_crosses_a_chunk(cc, sets):
    """n_gens = 1 and chunk + 3 rows that cycle through eight distinct inputs, one of them malformed: the oracle computes eight"""
    gens, handle = sets(1)
    chunk = CHUNK_ROWS
    assert "constexpr uint64_t T256_CHUNK_ROWS = 1u << 14;" in open(os.path.join(ROOT, "crescent-credentials_amd", "csrc", "t256commit.hip")).read()
    rng = random.Random(0xC4)
    rows = [([rng.randrange(Q)], rng.randrange(Q)) for _ in range(5)] + [([0], 0), ([Q], 1), ([1], 0)]
    n = chunk + 3
    scal, blind, want_out, want_status, want = cycled(gens, rows, n)
    out, status = call_rows(cc, handle, scal, blind, n)
    assert (status == want_status).all()
    assert (out.reshape(-1) == want_out).all()
    assert sorted(set(want_status.tolist())) == [MADE, MALFORMED] and want[5][1] == V.IDENTITY_COMPRESSED
    V.assert_both_parities([r for _, r in want])


def test_a_large_batch_shares_a_row_among_fewer_lanes(cc, sets):
    """16384 rows over 128 generators fill the chip at eight lanes a row (csrc/t256commit.hip's rule), four windows of every
    term a lane: the same bytes as at 64 lanes a row"""
    gens, handle = sets(128)
    rng = random.Random(0x1A7)
    rows = [([rng.randrange(Q) for _ in range(128)], rng.randrange(Q)) for _ in range(2)]
    rows += [(V.mixed_scalars(rng, 128), rng.randrange(Q)) for _ in range(5)] + [([0] * 128, 0)]
    n = 1 << 14
    scal, blind, want_out, want_status, want = cycled(gens, rows, n)
    out, status = call_rows(cc, handle, scal, blind, n)
    assert handle.commit_last_kernel_ms()[2] == 8
    assert (status == MADE).all() and (out.reshape(-1) == want_out).all()
    small, _ = call_rows(cc, handle, scal[:8 * 128 * 32], blind[:8 * 32], 8)
    assert handle.commit_last_kernel_ms()[2] == 64 and small.tobytes() == out[:8].tobytes()
    V.assert_both_parities([r for _, r in want])


def test_empty_calls(cc, sets):
    _, handle = sets(4)
    assert cc.lib().cg_t256_commit_rows_batch(handle._h, None, None, 0, None, None) == 0
    assert cc.lib().cg_hyrax_commit_batch(handle._h, 3, None, None, 0, None, None) == 0
    out, status = handle.commit_rows_batch(b"", b"")
    assert out.shape == (0, 33) and status.shape == (0,)


def test_two_handles_used_alternately(cc, sets):
    (g1, h1), (g4, h4) = sets(1), sets(4)
    rng = random.Random(0xA17)
    wants = []
    for _ in range(2):
        wants += check_rows(cc, g1, h1, [([rng.randrange(Q)], rng.randrange(Q)) for _ in range(3)])
        wants += check_rows(cc, g4, h4, [([rng.randrange(Q) for _ in range(4)], rng.randrange(Q)) for _ in range(3)])
    V.assert_both_parities([r for _, r in wants])
