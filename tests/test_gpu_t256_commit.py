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
CHUNK_SCALARS = 1 << 21     # its T256_CHUNK_SCALARS: the scalars of one launch set
TARGET_WAVES = 2048         # its T256_TARGET_WAVES: the waves below which a row keeps its lanes
COMMIT_SOURCE = os.path.join(ROOT, "crescent-credentials_amd", "csrc", "t256commit.hip")


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


@pytest.mark.parametrize("n", [3, 5, 12, 31, 33, 63, 65])
def test_rows_call_on_generator_counts_that_are_no_power_of_two(cc, sets, n):
    """3 and 63 make the n + 1 terms exactly W; 12 is the first count at sixteen lanes a row (two windows of a term a lane), 31
    has 32 lanes; 33 and 65 run a whole wave a row with the term index wrapping past W at an odd stride.  The blind sits on
    lane n mod W, and the scan's four-at-a-time steps meet the end of (n + 1) 2^log_per digits off a multiple of four"""
    gens, handle = sets(n)
    rng = random.Random(0x5100 + n)
    rows = [([rng.randrange(Q) for _ in range(n)], rng.randrange(Q)) for _ in range(3)]
    rows += [(V.mixed_scalars(rng, n), rng.randrange(Q)) for _ in range(3)]
    rows += [([0] * n, rng.randrange(1, Q)), ([0] * (n - 1) + [rng.randrange(1, Q)], 0), ([rng.randrange(1, Q)] + [0] * (n - 1), 0)]
    want = check_rows(cc, gens, handle, rows)
    assert all(st == MADE for st, _ in want)
    V.assert_both_parities([r for _, r in want])
    assert handle.commit_last_kernel_ms()[2] == min(64, 1 << n.bit_length())


def test_one_hot_digits_at_sixteen_lanes_a_row(cc, sets):
    """Twelve generators and the blind are 13 terms, W = 16: lane t has windows (t - j) mod 16 and that + 16 of term j.  One row
    for every term j and window w, whose only non-zero byte is byte w of term j's scalar: a wrong map from lane to window, or
    a wrong offset into the tables, fails at a named (j, w)"""
    n = 12
    gens, handle = sets(n)
    rng = random.Random(0x0E07)
    cells = [(j, w) for j in range(n + 1) for w in range(32)]
    digits = [rng.randrange(1, 256) for _ in cells]
    lo, hi = rng.sample(range(len(cells)), 2)
    digits[lo], digits[hi] = 1, 255
    assert len(cells) == 416 and 1 in digits and 255 in digits and all(1 <= d <= 255 for d in digits)
    terms = [[d << (8 * w) if i == j else 0 for i in range(n + 1)] for (j, w), d in zip(cells, digits)]
    ks = gens.ks + [gens.kh]
    want = [V.compressed(V.mul(d * ks[j] << (8 * w), V.G)) for (j, w), d in zip(cells, digits)]
    assert want[5] == gens.commit(terms[5][:n], terms[5][n])[1] and want[-1] == gens.commit(terms[-1][:n], terms[-1][n])[1]
    out, status = call_rows(cc, handle, pack([v for t in terms for v in t[:n]]), pack([t[n] for t in terms]), len(cells))
    assert handle.commit_last_kernel_ms()[2] == 16
    for i, (j, w) in enumerate(cells):
        assert status[i] == MADE and out[i].tobytes() == want[i], ("term %d window %d digit %d" % (j, w, digits[i]), out[i].tobytes().hex(), want[i].hex())
    V.assert_both_parities(want)


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


def test_the_check_kernel_past_its_first_sixty_four_elements(cc, sets):
    """num_vars = 7 is 128 scalars and 8 blinds a proof, and k_t256_check's wave takes them 64 at a time: elements 64 and 127
    (scalars) and 128 and 135 (blinds 0 and 7) are met on the second and third trip only.  Four proofs are bad in exactly one
    of these places, two are good"""
    num_vars = 7
    L, R = V.factored_lens(num_vars)
    assert (L, R) == (8, 16)
    gens, handle = sets(R)
    rng = random.Random(0xBAD3)
    proofs = [(V.mixed_scalars(rng, L * R) if i % 2 else [rng.randrange(Q) for _ in range(L * R)], [rng.randrange(Q) for _ in range(L)]) for i in range(6)]
    proofs[0][0][64] = Q
    proofs[2][0][127] = (1 << 256) - 1
    proofs[3][1][0] = (1 << 256) - 1
    proofs[5][1][7] = Q
    want = [V.hyrax(gens, num_vars, v, b) for v, b in proofs]
    assert [st for st, _ in want] == [MALFORMED, MADE, MALFORMED, MALFORMED, MADE, MALFORMED]
    assert all(rows == V.ZERO_ROW * L for st, rows in want if st == MALFORMED)
    out, status = call_hyrax(cc, handle, num_vars, pack([x for v, _ in proofs for x in v]), pack([x for _, b in proofs for x in b]), 6)
    for i, (st, rows) in enumerate(want):
        assert status[i] == st and out[i].tobytes() == rows, i
    V.assert_both_parities([out[i, j].tobytes() for i in (1, 4) for j in range(L)])


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
    assert "constexpr uint64_t T256_CHUNK_ROWS = 1u << 14;" in open(COMMIT_SOURCE).read()
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


def lanes_of(rows, n_terms):
    """csrc/t256commit.hip's pick_log_w, restated: the least power of two >= n_terms, at most 64, halved while the rows still
    make TARGET_WAVES waves of 64 lanes at half the width"""
    log_w = 0
    while log_w < 6 and (1 << log_w) < n_terms:
        log_w += 1
    while log_w > 0 and (rows << (log_w - 1)) >> 6 >= TARGET_WAVES:
        log_w -= 1
    return 1 << log_w


def test_the_halved_widths_on_many_terms(cc, sets):
    """33 generators are 34 terms, 64 lanes a row for a small call.  A call halves W while rows · W / 2 / 64 >= 2048 waves:
    4096 rows · 32 / 64 = 2048, so 4096 rows run at W = 32 (and 4096 · 16 / 64 = 1024 stops there); 8192 rows go on to W = 16
    (8192 · 16 / 64 = 2048, 8192 · 8 / 64 = 1024); 16384 rows to W = 8 (16384 · 8 / 64 = 2048, 16384 · 4 / 64 = 1024).
    W = 32 with 34 terms is the lane-to-window map with log_per = 0 and a term index that wraps past W; W = 16 has two windows
    of a term a lane, W = 8 four.  All three are one chunk.  The same bytes as at 64 lanes a row"""
    n_gens = 33
    gens, handle = sets(n_gens)
    assert "constexpr uint64_t T256_TARGET_WAVES = 2048;" in open(COMMIT_SOURCE).read()
    assert [lanes_of(r, n_gens + 1) for r in (8, 4095, 4096, 8191, 8192, 16383, 16384)] == [64, 64, 32, 32, 16, 16, 8]
    rng = random.Random(0x1A8)
    rows = [([rng.randrange(Q) for _ in range(n_gens)], rng.randrange(Q)) for _ in range(2)]
    rows += [(V.mixed_scalars(rng, n_gens), rng.randrange(Q)) for _ in range(5)] + [([0] * n_gens, 0)]
    scal, blind, want_out, want_status, want = cycled(gens, rows, 16384)
    assert (want_status == MADE).all() and want[7][1] == V.IDENTITY_COMPRESSED
    V.assert_both_parities([r for _, r in want])
    small, small_status = call_rows(cc, handle, scal[:8 * n_gens * 32], blind[:8 * 32], 8)
    assert handle.commit_last_kernel_ms()[2] == 64
    assert (small_status == MADE).all() and (small.reshape(-1) == want_out[:8 * 33]).all()
    for n, lanes in ((4096, 32), (8192, 16), (16384, 8)):
        out, status = call_rows(cc, handle, scal[:n * n_gens * 32], blind[:n * 32], n)
        assert handle.commit_last_kernel_ms()[2] == lanes, n
        assert (status == MADE).all() and (out.reshape(-1) == want_out[:n * 33]).all(), n
        assert out[:8].tobytes() == small.tobytes(), n


def cycled_proofs(gens, num_vars, proofs, order):
    """the proofs `proofs[i] for i in order` as one call's arrays, and what the oracle makes of the distinct ones:
    (vars, blinds, expected bytes, expected statuses, want)"""
    want = [V.hyrax(gens, num_vars, v, b) for v, b in proofs]
    vars_ = [pack(v) for v, _ in proofs]
    blinds = [pack(b) for _, b in proofs]
    outs = [np.frombuffer(rows, np.uint8) for _, rows in want]
    return (np.concatenate([vars_[i] for i in order]), np.concatenate([blinds[i] for i in order]), np.concatenate([outs[i] for i in order]),
            np.array([want[i][0] for i in order], np.uint8), want)


def test_a_hyrax_call_that_crosses_a_row_bound_chunk(cc, sets):
    """num_vars = 3 is two rows of four scalars a proof: a chunk is min(16384 / 2, 2^21 / 8) = 8192 proofs, bound by its rows.
    8192 + 5 proofs cycle through seven distinct ones; 7 does not divide 8192, so the second chunk starts at another place of
    the cycle than the first: proof 8192 is the cycle's place 2.  Place 2 is malformed by a scalar, place 3 all zero with
    zero blinds (the identity's bytes), place 5 malformed by a blind: the second chunk, places 2 to 6, holds all three.  What
    the second chunk reads (scalars and blinds from proof 8192 on) and writes (rows from 2 · 8192 on, statuses from 8192 on)
    is offset by whole proofs, and its flags are indexed from the chunk's first proof"""
    num_vars = 3
    L, R = V.factored_lens(num_vars)
    gens, handle = sets(R)
    per_chunk = min(CHUNK_ROWS // L, CHUNK_SCALARS // (L * R))
    assert (L, R, per_chunk) == (2, 4, 8192) and CHUNK_ROWS // L < CHUNK_SCALARS // (L * R)
    rng = random.Random(0xC5)
    proofs = [([rng.randrange(Q) for _ in range(L * R)], [rng.randrange(Q) for _ in range(L)]) for _ in range(7)]
    proofs[1] = (V.mixed_scalars(rng, L * R), proofs[1][1])
    proofs[2][0][5] = Q
    proofs[3] = ([0] * (L * R), [0] * L)
    proofs[5][1][1] = (1 << 256) - 1
    n = per_chunk + 5
    order = [i % 7 for i in range(n)]
    vars_, blinds, want_out, want_status, want = cycled_proofs(gens, num_vars, proofs, order)
    assert [st for st, _ in want] == [MADE, MADE, MALFORMED, MADE, MADE, MALFORMED, MADE] and want[3][1] == V.IDENTITY_COMPRESSED * L
    assert order[per_chunk] == 2 and order[per_chunk:] == [2, 3, 4, 5, 6] and order[:5] != order[per_chunk:]
    assert {MADE, MALFORMED} == set(want_status[per_chunk:].tolist())
    out, status = call_hyrax(cc, handle, num_vars, vars_, blinds, n)
    assert (status == want_status).all()
    assert out.size == n * L * 33 and (out.reshape(-1) == want_out).all()
    V.assert_both_parities([rows[33 * j:33 * j + 33] for _, rows in want for j in range(L)])


def test_a_hyrax_call_that_crosses_a_scalar_bound_chunk(cc, sets):
    """num_vars = 16 is 256 rows of 256 scalars a proof: a chunk is min(16384 / 256, 2^21 / 65536) = min(64, 32) = 32 proofs,
    bound by its scalars, so the 33rd proof is a chunk of its own.  The proofs cycle through three distinct ones of a circuit's
    mix of wires, the second of them malformed (the oracle's 2 · 256 rows take three seconds; a fourth proof would add half as
    much again): the 33rd is the third distinct proof, so its rows are neither those of proof 0 nor those of proof 1, which
    a chunk-relative offset would read or write"""
    num_vars = 16
    L, R = V.factored_lens(num_vars)
    gens, handle = sets(R)
    source = open(COMMIT_SOURCE).read()
    assert "constexpr uint64_t T256_CHUNK_SCALARS = 1u << 21;" in source and "constexpr uint64_t T256_CHUNK_ROWS = 1u << 14;" in source
    per_chunk = min(CHUNK_ROWS // L, CHUNK_SCALARS // (L * R))
    assert (L, R, per_chunk) == (256, 256, 32) and CHUNK_SCALARS // (L * R) < CHUNK_ROWS // L
    rng = random.Random(0xC6)
    proofs = [(V.mixed_scalars(rng, L * R), [rng.randrange(Q) for _ in range(L)]) for _ in range(3)]
    proofs[1][0][L * R - R - 1] = Q                                             # the last scalar of the last row but one
    n = per_chunk + 1
    order = [i % 3 for i in range(n)]
    vars_, blinds, want_out, want_status, want = cycled_proofs(gens, num_vars, proofs, order)
    assert vars_.size == n << (num_vars + 5) and [st for st, _ in want] == [MADE, MALFORMED, MADE]
    assert want[2][1] != want[0][1] and want[2][1] != want[1][1] and order[per_chunk] == 2 and (order[0], order[1]) == (0, 1)
    out, status = call_hyrax(cc, handle, num_vars, vars_, blinds, n)
    assert status[per_chunk] == MADE and out[per_chunk].tobytes() == want[2][1]
    assert out[per_chunk].tobytes() != out[0].tobytes() and out[per_chunk].tobytes() != out[1].tobytes()
    assert (status == want_status).all()
    assert (out.reshape(-1) == want_out).all()
    V.assert_both_parities([rows[33 * j:33 * j + 33] for _, rows in want for j in range(L)])


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
