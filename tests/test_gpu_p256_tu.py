"""pi2's public inputs on the GPU (csrc/p256tu.hip: cg_p256_tu_batch, cg_p256_rtu_batch; csrc/p256.hpp, csrc/fq256.hpp,
csrc/fp256.hpp): `compute_TU` and `compute_RTU` on P-256 for batches of rows under one handle.

Expected bytes and statuses come from tests/p256_vectors.py, a pure-Python restatement over integers that shares no code with
the library (tests/test_p256_cpu.py holds it against the NIST example).  Every comparison is byte for byte, statuses
included.  The oracle's rows are computed once per module; the batch that crosses a chunk tiles them."""
import random
import re
import os

import numpy as np
import pytest

import p256_vectors as V
import poseidon_vectors as PV
import test_gpu_device_link_make as M
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

N, P, G = V.N, V.P, V.G
MADE, MALFORMED, BAD_SIGNATURE = 1, 2, 3
INVALID_ARGUMENT = -1
K = load_golden("p256_ecdsa_kats.json")
as_point = lambda b: None if b == V.ZERO_POINT else (int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big"))


def chunk_size():
    src = open(os.path.join(ROOT, "crescent-credentials_amd", "csrc", "p256tu.hip")).read()
    return eval(re.search(r"constexpr uint64_t P256CHUNK = ([0-9u<> ]+);", src).group(1).replace("u", ""))


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


@pytest.fixture(scope="module")
def world(cc):
    w = M.World(cc, "mdl", 0x9256)
    yield w
    w.pvk.close()


def kat_row():
    return (V.point_bytes((int(K["q_x"], 16), int(K["q_y"], 16))), V.be(int(K["r"], 16)) + V.be(int(K["s"], 16)), bytes.fromhex(K["digest"]))


class Rows:
    """rows (q_xy, sig, digest) with what the oracle makes of them, computed once"""

    def __init__(self, rows):
        self.rows = list(rows)
        self.want = [V.compute_rtu(*row) for row in self.rows]          # (status, r_xy, t_xy, u_xy)

    def packed(self, idx=None):
        rows = self.rows if idx is None else [self.rows[i] for i in idx]
        return [b"".join(r[j] for r in rows) for j in range(3)]


@pytest.fixture(scope="module")
def honest():
    """67 valid rows: the NIST example, Q = G, Q = -G, a row whose final sum is a doubling, and 63 seeded signatures"""
    rng = random.Random(0x67)
    special = [kat_row()]
    for priv in (1, N - 1):
        dg = bytes(rng.randrange(256) for _ in range(32))
        Q, r, s = V.sign(priv, dg, rng.randrange(1, N))
        special.append((V.point_bytes(Q), V.be(r) + V.be(s), dg))
    special.append(V.coincident_row(0x1234567, 0xC0FFEE))
    h = Rows(special + V.signed_rows(0x6767, 63))
    assert len(h.rows) == 67 and all(w[0] == MADE for w in h.want)
    return h


def check_rtu(got, want):
    r, t, u, status = got
    assert len(status) == len(want)
    for i, (st, r_xy, t_xy, u_xy) in enumerate(want):
        assert (int(status[i]), r[i].tobytes(), t[i].tobytes(), u[i].tobytes()) == (st, r_xy, t_xy, u_xy), i


# ---- 1. the recorded example ------------------------------------------------------------------------------------------------------
def test_the_nist_example_through_both_calls(world):
    G16 = world.cc.Groth16
    q, sig, dg = kat_row()
    r, t, u, status = G16.p256_rtu_batch(world.pvk, q, sig, dg)
    assert status.tolist() == [MADE]
    assert r[0].tobytes().hex() == K["r"] + K["r_y"]
    assert (MADE, r[0].tobytes(), t[0].tobytes(), u[0].tobytes()) == V.compute_rtu(q, sig, dg)
    # s T + U = Q: what the circuit will check
    T, U = as_point(t[0].tobytes()), as_point(u[0].tobytes())
    assert V.add(V.mul(int(K["s"], 16), T), U) == as_point(q)
    t2, u2, status2 = G16.p256_tu_batch(world.pvk, r[0], dg)
    assert status2.tolist() == [MADE] and np.array_equal(t2, t) and np.array_equal(u2, u)
    # and on Python integers
    R = (int(K["r"], 16), int(K["r_y"], 16))
    assert G16.p256_rtu(world.pvk, [(as_point(q), int(K["r"], 16), int(K["s"], 16), int(K["digest"], 16))]) == [(MADE, (R, T, U))]
    assert G16.p256_tu(world.pvk, [(R, int(K["digest"], 16))]) == [(T, U)]


# ---- 2. one row, a partial wave, a chunk boundary ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 67])
def test_batches_equal_the_oracle_and_tu_after_rtu_returns_the_provers_points(world, honest, n):
    """n = 67 spans a partial wave: 67 rows are two waves of the scalar and finishing stages, and their terms straddle waves"""
    G16 = world.cc.Groth16
    idx = list(range(n)) if n > 1 else [4]
    got = G16.p256_rtu_batch(world.pvk, *honest.packed(idx))
    check_rtu(got, [honest.want[i] for i in idx])
    r, t, u, _ = got
    t2, u2, status2 = G16.p256_tu_batch(world.pvk, r.reshape(-1), honest.packed(idx)[2])
    assert status2.tolist() == [MADE] * n and np.array_equal(t2, t) and np.array_equal(u2, u)


def test_across_a_chunk_with_bad_rows_at_its_edges(world, honest):
    """There is no hook that lowers the chunk size, so this is the smallest batch that crosses a chunk: chunk + 1 rows, the 67
    rows of the oracle tiled, with a malformed row or a bad signature on either side of the boundary"""
    G16 = world.cc.Groth16
    chunk = chunk_size()
    assert chunk == 1 << 14
    n = chunk + 1
    tile = np.arange(n) % 67
    q, sig, dg = [np.frombuffer(b, np.uint8).reshape(67, -1)[tile].copy() for b in honest.packed()]
    want = [np.frombuffer(b"".join(w[j] for w in honest.want), np.uint8).reshape(67, 64)[tile].copy() for j in (1, 2, 3)]
    want_status = np.full(n, MADE, np.uint8)
    q[0, 63] ^= 1                                                           # Q off the curve
    sig[chunk - 1, :32] = np.frombuffer(V.be(int.from_bytes(sig[chunk - 1, :32].tobytes(), "big") - 1), np.uint8)
    sig[chunk, 32:] = 0                                                     # s = 0
    for i, st in ((0, MALFORMED), (chunk - 1, BAD_SIGNATURE), (chunk, MALFORMED)):
        assert V.compute_rtu(q[i].tobytes(), sig[i].tobytes(), dg[i].tobytes())[0] == st
        want_status[i] = st
        for a in want:
            a[i] = 0
    r, t, u, status = G16.p256_rtu_batch(world.pvk, q.reshape(-1), sig.reshape(-1), dg.reshape(-1))
    assert np.array_equal(status, want_status)
    for got, w in zip((r, t, u), want):
        assert np.array_equal(got, w)
    # the relying party's call on the same rows: R is the prover's, a zeroed R is (0, 0) and off the curve
    t2, u2, status2 = G16.p256_tu_batch(world.pvk, r.reshape(-1), dg.reshape(-1))
    assert np.array_equal(status2, np.where(want_status == MADE, MADE, MALFORMED))
    assert np.array_equal(t2, want[1]) and np.array_equal(u2, want[2])


# ---- 3. good rows beside bad rows ----------------------------------------------------------------------------------------------------
def test_mixed_batches_touch_only_their_bad_rows(world, honest):
    G16 = world.cc.Groth16
    good = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
    q0, sig0, dg0 = honest.rows[12]
    r0, s0 = int.from_bytes(sig0[:32], "big"), int.from_bytes(sig0[32:], "big")
    qy = int.from_bytes(q0[32:], "big")
    bad_rtu = [
        ((q0, V.be(0) + sig0[32:], dg0), MALFORMED),                        # r = 0
        ((q0, V.be(N) + sig0[32:], dg0), MALFORMED),                        # r = n: 0 mod n, and not below n
        ((q0, sig0[:32] + V.be(0), dg0), MALFORMED),                        # s = 0
        ((q0, sig0[:32] + V.be(N), dg0), MALFORMED),                        # s = n
        ((q0[:32] + V.be(qy + 1), sig0, dg0), MALFORMED),                   # Q off the curve
        ((V.be(P) + q0[32:], sig0, dg0), MALFORMED),                        # Q.x >= p
        ((q0, V.be(r0 - 1) + sig0[32:], dg0), BAD_SIGNATURE),               # r - 1
        (V.coincident_row(0x1234567, 0xBEEF, opposite=True), BAD_SIGNATURE),     # u G = -(v Q): R is the identity
        (V.coincident_row(1, 0xBEEF, opposite=True), BAD_SIGNATURE),        # the same with Q = G
    ]
    uG, vQ = V.terms_of(*bad_rtu[7][0])
    assert uG == V.neg(vQ) and uG is not None
    rows, want = [], []
    for i, (row, st) in enumerate(bad_rtu):                                 # good and bad rows alternate
        rows += [honest.rows[good[i]], row]
        want += [honest.want[good[i]], (st,) + (V.ZERO_POINT,) * 3]
        assert V.compute_rtu(*row) == want[-1], i
    rows.append(honest.rows[good[9]])
    want.append(honest.want[good[9]])
    check_rtu(G16.p256_rtu_batch(world.pvk, *[b"".join(r[j] for r in rows) for j in range(3)]), want)

    # compute_TU: R.x >= p, R off the curve (y + 1), digest = 0 (U is zero bytes, MADE), a digest >= n
    r_xy = honest.want[12][1]
    ry = int.from_bytes(r_xy[32:], "big")
    tu_rows = [(honest.want[1][1], honest.rows[1][2]), (V.be(P) + r_xy[32:], dg0), (honest.want[2][1], honest.rows[2][2]),
               (r_xy[:32] + V.be(ry + 1), dg0), (r_xy, bytes(32)), (V.be((1 << 256) - 1) + r_xy[32:], dg0), (r_xy, V.be(N + 5)),
               (r_xy[:32] + V.be(P), dg0), (honest.want[3][1], honest.rows[3][2])]
    want_tu = [V.compute_tu(*row) for row in tu_rows]
    assert [w[0] for w in want_tu] == [MADE, MALFORMED, MADE, MALFORMED, MADE, MALFORMED, MADE, MALFORMED, MADE]
    assert want_tu[4][2] == V.ZERO_POINT and want_tu[4][1] != V.ZERO_POINT and want_tu[6] == V.compute_tu(r_xy, V.be(5))
    t, u, status = G16.p256_tu_batch(world.pvk, b"".join(r[0] for r in tu_rows), b"".join(r[1] for r in tu_rows))
    for i, w in enumerate(want_tu):
        assert (int(status[i]), t[i].tobytes(), u[i].tobytes()) == w, i


# ---- 4. what a signer can arrange -------------------------------------------------------------------------------------------------------
def test_signer_chosen_coincidences_go_through_the_general_addition(world, honest):
    """Q = G, Q = -G, u G = v Q (the final sum is a doubling) and u G = -(v Q) (it is the identity): an incomplete addition
    gets these rows wrong.  Each row is first shown, with the oracle, to hit its case."""
    G16 = world.cc.Groth16
    rows = [honest.rows[1], honest.rows[2]]
    assert as_point(rows[0][0]) == G and as_point(rows[1][0]) == V.neg(G)
    for priv in (1, N - 1, 0x1234567, 5):
        row = V.coincident_row(priv, 0xD0B1E + priv % 7)
        uG, vQ = V.terms_of(*row)
        assert uG == vQ and uG is not None and V.compute_rtu(*row)[0] == MADE
        rows.append(row)
        row = V.coincident_row(priv, 0xD0B1E + priv % 7, opposite=True)
        uG, vQ = V.terms_of(*row)
        assert uG == V.neg(vQ) and uG is not None and V.compute_rtu(*row)[0] == BAD_SIGNATURE
        rows.append(row)
    want = [V.compute_rtu(*row) for row in rows]
    assert [w[0] for w in want] == [MADE, MADE] + [MADE, BAD_SIGNATURE] * 4
    check_rtu(G16.p256_rtu_batch(world.pvk, *[b"".join(r[j] for r in rows) for j in range(3)]), want)


# ---- 5. argument errors ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_touch_nothing(world, honest):
    L = world.cc.lib()
    ins = [np.frombuffer(b, np.uint8).copy() for b in honest.packed([0])]
    outs = [np.full(64, 0xA5, np.uint8) for _ in range(3)] + [np.full(1, 0xA5, np.uint8)]
    p = lambda a: a.ctypes.data
    full = [p(a) for a in ins] + [1] + [p(a) for a in outs]
    for j in (0, 1, 2, 4, 5, 6, 7):
        args = list(full)
        args[j] = None
        assert L.cg_p256_rtu_batch(world.pvk._h, *args) == INVALID_ARGUMENT and b"null" in L.cg_last_error(), j
    full_tu = [p(ins[0]), p(ins[2]), 1, p(outs[1]), p(outs[2]), p(outs[3])]
    for j in (0, 1, 3, 4, 5):
        args = list(full_tu)
        args[j] = None
        assert L.cg_p256_tu_batch(world.pvk._h, *args) == INVALID_ARGUMENT and b"null" in L.cg_last_error(), j
    assert L.cg_p256_rtu_batch(world.pvk._h, None, None, None, 0, None, None, None, None) == 0
    assert L.cg_p256_tu_batch(world.pvk._h, None, None, 0, None, None, None) == 0
    assert all((a == 0xA5).all() for a in outs)
    G16 = world.cc.Groth16
    assert [a.shape for a in G16.p256_rtu_batch(world.pvk, b"", b"", b"")] == [(0, 64)] * 3 + [(0,)]
    assert G16.p256_tu(world.pvk, []) == [] and G16.p256_rtu(world.pvk, []) == []
    with pytest.raises(ValueError):
        G16.p256_tu_batch(world.pvk, bytes(64), bytes(31))


# ---- 6. the handle's state --------------------------------------------------------------------------------------------------------------
def test_the_table_goes_up_once_and_h_q_calls_in_between_evict_nothing(cc, honest):
    w = M.World(cc, "mdl", 0x9257)
    try:
        G16 = cc.Groth16
        assert w.pvk.p256_last_kernel_ms() == (0.0, 0.0, 0.0, 0)
        idx = list(range(5))
        first = G16.p256_rtu_batch(w.pvk, *honest.packed(idx))
        check_rtu(first, [honest.want[i] for i in idx])
        *ms, uploads = w.pvk.p256_last_kernel_ms()
        assert all(t > 0 for t in ms) and uploads == 1
        # h_Q on the same handle, larger than the P-256 batch, then the relying party's call, then the prover's again
        rng = random.Random(0x57A8)
        many = [tuple(rng.randrange(PV.BN254_FR) for _ in range(3)) for _ in range(200)]
        triple = lambda q: b"".join(int(x).to_bytes(32, "little") for x in q)
        h, _ = G16.hq_batch_packed(w.pvk, b"".join(triple(q) for q in many))
        assert h[199].tobytes() == PV.hq(*many[199]) and h[0].tobytes() == PV.hq(*many[0])
        t2, u2, status2 = G16.p256_tu_batch(w.pvk, first[0].reshape(-1), honest.packed(idx)[2])
        assert status2.tolist() == [MADE] * 5 and np.array_equal(t2, first[1]) and np.array_equal(u2, first[2])
        again = G16.p256_rtu_batch(w.pvk, *honest.packed(idx))
        assert all(np.array_equal(a, b) for a, b in zip(again, first))
        h2, _ = G16.hq_batch_packed(w.pvk, triple(many[7]))
        assert h2[0].tobytes() == PV.hq(*many[7])
        *ms, uploads = w.pvk.p256_last_kernel_ms()
        assert all(t > 0 for t in ms) and uploads == 1
        assert w.pvk.hq_last_kernel_ms()[2] == 1
    finally:
        w.pvk.close()
