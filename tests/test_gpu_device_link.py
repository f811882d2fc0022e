"""The BN254 half of device proofs on the GPU (csrc/devicelink.hip: cg_device_link_verify_batch; csrc/device_link.hpp,
csrc/sha256.hpp): `DeviceProof::verify` (creds/src/device.rs:168-213) short of pi2 for batches of device-bound showings.

Proofs are made and judged by tests/device_link_vectors.py, a pure-Python restatement that shares no code with the library and
reads the BYTES the call takes; every expected verdict, part and digest comes from it.  Two layouts: [COMMITTED, HIDDEN,
COMMITTED, COMMITTED, REVEALED] with the device keys at inputs 2 and 3, and [COMMITTED, COMMITTED, HIDDEN, COMMITTED] with them
at inputs 1 and 0, so that the committed indices are derived and not assumed.

On the coincident sums: which partial sums a valid proof can make coincide is limited by the transcripts.  The first two
fixed-base partials of a k always sum to k - c y, so they are OPPOSITE only where k = c y with c a hash of k: out of reach.  They
are EQUAL where the nonces are moved along the line that keeps k fixed (doubling_record).  A cancellation is reached with
every nonce zero (each k's last addition meets its opposite and k is O) and with zero blindings (lhs1's last addition cancels to
O, and so does the fourth of pi1's k_0, whose fifth restarts from O)."""
import ctypes
import os
import random
import re
from types import SimpleNamespace

import numpy as np
import pytest

import device_link_vectors as D
import verify_vectors as V
from conftest import ROOT

pytestmark = pytest.mark.gpu

o = D.o
R, Q = D.R, D.Q
REJECT, ACCEPT, MALFORMED = D.REJECT, D.ACCEPT, D.MALFORMED
INVALID_ARGUMENT, MALFORMED_KEY = -1, -6
COM, HID, REV = D.COMMITTED, D.HIDDEN, D.REVEALED
LAYOUTS = {"mdl": ([COM, HID, COM, COM, REV], 2, 3), "keys first": ([COM, COM, HID, COM], 1, 0)}
inv = lambda v: pow(v, R - 2, R)


def chunk_size():
    src = open(os.path.join(ROOT, "crescent-credentials_amd", "csrc", "devicelink.hip")).read()
    return eval(re.search(r"constexpr uint64_t DLCHUNK = ([0-9u<> ]+);", src).group(1).replace("u", ""))


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


class World:
    """one synthetic key under a layout, loaded on the GPU, with eight honest records and the restatement's answers cached"""

    def __init__(self, cc, name, seed):
        io, pos0, pos1 = LAYOUTS[name]
        self.cc, self.key = cc, D.make_key(io, pos0, pos1, seed)
        self.pvk = cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(self.key.vk)))
        self.rng = random.Random(seed ^ 0xD0)
        self.recs = [D.random_record(self.key, self.rng) for _ in range(8)]
        self._answers = {}

    def row(self, rec):
        return D.record_bytes(self.key, rec)

    def want(self, row):
        if row not in self._answers:
            self._answers[row] = D.verify(self.key, row)
        return self._answers[row]

    def call(self, rows, h_len=32):
        k = self.key
        return self.cc.Groth16.device_link_verify_batch_packed(self.pvk, k.io, k.pos0, k.pos1, *D.pack(rows), h_len=h_len)

    def check(self, rows, h_len=32, names=None):
        """the call's three outputs against the restatement, row by row; returns the verdicts"""
        verdicts, parts, e = self.call(rows, h_len)
        for i, row in enumerate(rows):
            v, p, d = self.want(row)
            name = (names[i] if names else i, v)
            assert int(verdicts[i]) == v, name
            assert tuple(int(x) for x in parts[i]) == p, name
            assert e[i].tobytes() == d, name
        return [int(v) for v in verdicts]


@pytest.fixture(scope="module", params=list(LAYOUTS))
def world(request, cc):
    w = World(cc, request.param, 0xDE71CE + len(request.param))
    yield w
    w.pvk.close()


@pytest.fixture(scope="module")
def mdl(cc):
    w = World(cc, "mdl", 0x3D1)
    yield w
    w.pvk.close()


def but(rec, **kw):
    d = dict(vars(rec))
    d.update(kw)
    return SimpleNamespace(**d)


# ---- honest proofs ---------------------------------------------------------------------------------------------------------------
def test_one_honest_proof(world):
    assert world.check([world.row(world.recs[0])]) == [ACCEPT]
    assert world.want(world.row(world.recs[0])) == (ACCEPT, (ACCEPT, ACCEPT), world.recs[0].digest)


def test_a_wave_and_one_lane(world):
    rows = [world.row(world.recs[i % 8]) for i in range(65)]
    assert world.check(rows) == [ACCEPT] * 65


def test_more_than_a_chunk_with_forged_rows_at_its_edges(mdl):
    chunk = chunk_size()
    assert chunk == 1 << 15
    n = chunk + 1
    rows = [mdl.row(r) for r in mdl.recs]
    forged = mdl.row(but(mdl.recs[3], m=(mdl.recs[3].m + 1) % R))
    assert mdl.want(forged)[0] == REJECT
    at = (0, chunk - 1, chunk)
    cols = [np.frombuffer(D.pack(rows)[j], np.uint8).reshape(8, -1) for j in range(9)]
    idx = np.arange(n) % 8
    arrays = [c[idx].copy() for c in cols]
    for i in at:
        for j in range(9):
            arrays[j][i] = np.frombuffer(forged[j], np.uint8)
    k = mdl.key
    verdicts, parts, e = mdl.cc.Groth16.device_link_verify_batch_packed(mdl.pvk, k.io, k.pos0, k.pos1, *[a.reshape(-1) for a in arrays], h_len=32)
    want = [mdl.want(r) for r in rows]
    want_v = np.array([w[0] for w in want], np.uint8)[idx]
    want_p = np.array([w[1] for w in want], np.uint8)[idx]
    want_e = np.stack([np.frombuffer(w[2], np.uint8) for w in want])[idx]
    fv, fp, fd = mdl.want(forged)
    for i in at:
        want_v[i], want_p[i], want_e[i] = fv, fp, np.frombuffer(fd, np.uint8)
    assert (want_v == ACCEPT).sum() == n - 3
    assert np.array_equal(verdicts, want_v) and np.array_equal(parts, want_p) and np.array_equal(e, want_e)


# ---- the digest -------------------------------------------------------------------------------------------------------------------
def test_digest_at_every_padding_boundary(mdl):
    """one record's commitments under h_Q of the lengths that put the message's end at 55, 56, 63, 0 and 1 mod 64"""
    rng = random.Random(0x9AD)
    args = dict(q0=rng.randrange(R), r0=rng.randrange(R), q1=rng.randrange(R), r1_orig=rng.randrange(R), r1=rng.randrange(R), z=rng.randrange(R),
                tz=rng.randrange(R), nonces0=[rng.randrange(R) for _ in range(3)], nonces1=[rng.randrange(R) for _ in range(3)])
    first = D.prove(mdl.key, h_q=b"", **args)
    base = len(D.message(first.pi0_c, first.com0, first.com1, first.comz, b""))
    seen = set()
    for want_mod in (55, 56, 63, 0, 1):
        h_len = (want_mod - base) % 64
        rec = D.prove(mdl.key, h_q=bytes(rng.randrange(256) for _ in range(h_len)), **args)
        assert len(D.message(rec.pi0_c, rec.com0, rec.com1, rec.comz, rec.h_q)) % 64 == want_mod and 0 <= h_len <= 64
        assert mdl.check([mdl.row(rec)] * 2, h_len=h_len) == [ACCEPT] * 2
        seen.add(want_mod)
    assert len(seen) == 5


def test_text_edges_of_the_challenge(mdl):
    """pi0.c of 0 (the empty string), 1, 10^9 (a chunk of zeros), 10^18 - 1 and r - 1: rejected, and the digest still the
    restatement's"""
    rec = mdl.recs[0]
    values = [0, 1, 10**9, 10**18 - 1, R - 1]
    rows = [mdl.row(but(rec, pi0_c=v)) for v in values]
    assert len({mdl.want(r)[2] for r in rows}) == 5
    assert mdl.check(rows, names=values) == [REJECT] * 5


def steered_records(w):
    """valid proofs whose commitments have the text forms "(1, 2)" and "infinity" """
    k, rng = w.key, random.Random(0x57EE)
    z = rng.randrange(1, R)
    gen = D.random_record(k, rng, z=z, tz=(1 - z * k.kg) * inv(k.kh) % R)
    assert gen.comz == o.G1_GEN
    comz_o = D.random_record(k, rng, z=0, tz=0)
    assert comz_o.comz is None
    com1_o = D.random_record(k, rng, q1=0, r1=0)
    assert com1_o.com1 is None and com1_o.com1_orig is not None
    return [("comz = (1, 2)", gen), ("comz = O", comz_o), ("com1 = O", com1_o)]


def test_text_edges_of_the_points(mdl):
    cases = steered_records(mdl)
    rows = [mdl.row(r) for _, r in cases]
    assert b"(1, 2)" in D.message(cases[0][1].pi0_c, cases[0][1].com0, cases[0][1].com1, cases[0][1].comz, b"")
    assert D.message(cases[1][1].pi0_c, cases[1][1].com0, cases[1][1].com1, None, b"").endswith(b"infinity")
    assert mdl.check(rows, names=[n for n, _ in cases]) == [ACCEPT] * 3


# ---- coincident and cancelling sums ----------------------------------------------------------------------------------------------
def doubling_record(w):
    """nonces moved along the lines that keep pi0's k_0, k_1 and pi1's k_1 fixed until s00 g' = s01 h and u0 g = u1 h: the second
    addition of both sums is a doubling"""
    k, rng = w.key, random.Random(0xD0B1)
    s = lambda: rng.randrange(1, R)
    sec = dict(q0=s(), r0=s(), q1=s(), r1_orig=s(), r1=s(), z=s(), tz=s(), h_q=bytes(32))
    kap0, kap1, kap2, n0 = s(), s(), s(), s()

    def on_lines(a, n1):
        return dict(nonces0=(a, (kap0 - a * k.kgp) * inv(k.kh) % R, (kap1 - a * k.kg) * inv(k.kh) % R), nonces1=(n0, n1, (kap2 - n1 * k.kg) * inv(k.kh) % R))

    first = D.prove(k, **sec, **on_lines(s(), s()))
    c0, c1 = first.pi0_c, first.pi1_c
    a = (kap0 - c0 * sec["r1_orig"] * k.kh + c0 * sec["q1"] * k.kgp) * inv(2 * k.kgp) % R
    n1 = (kap2 - c1 * sec["tz"] * k.kh + c1 * sec["z"] * k.kg) * inv(2 * k.kg) % R
    rec = D.prove(k, **sec, **on_lines(a, n1))
    assert (rec.pi0_c, rec.pi1_c) == (c0, c1)
    assert rec.pi0_s[0] * k.kgp % R == rec.pi0_s[1] * k.kh % R != 0 and rec.pi1_s[1] * k.kg % R == rec.pi1_s[2] * k.kh % R != 0
    return rec


def m_record(w, target):
    """com0 kept as a point while its opening moves along the line, until m = q0 + q1 e1 + z e2 is `target`"""
    k, rng = w.key, random.Random(0x3E7 + target % 7)
    s = lambda: rng.randrange(1, R)
    ups = s()
    args = dict(q1=s(), r1_orig=s(), r1=s(), z=s(), tz=s(), nonces0=(s(), s(), s()), nonces1=(s(), s(), s()), h_q=bytes(range(32)))
    split = lambda q0: dict(q0=q0, r0=(ups - q0 * k.kg) * inv(k.kh) % R)
    first = D.prove(k, **args, **split(s()))
    e1, e2 = D.e_of(first.digest)
    rec = D.prove(k, **args, **split((target - args["q1"] * e1 - args["z"] * e2) % R))
    assert rec.m == target and rec.com0 == first.com0 and rec.digest == first.digest
    return rec


def test_coincident_and_cancelling_sums(world):
    k, rng = world.key, random.Random(0xCA9C)
    zero_nonces = D.random_record(k, rng, nonces0=(0, 0, 0), nonces1=(0, 0, 0))
    zero_blindings = D.random_record(k, rng, r0=0, r1=0, tz=0)
    e1, e2 = D.e_of(zero_blindings.digest)
    assert D.add(D.add(zero_blindings.com0, D.mul(zero_blindings.com1, e1)), D.mul(zero_blindings.comz, e2)) == D.mul(k.g, zero_blindings.m)   # lhs1 = O
    cases = [("every k is O", zero_nonces), ("doublings", doubling_record(world)), ("lhs1 = O by a cancellation", zero_blindings),
             ("m = 0", m_record(world, 0)), ("m = r - 1", m_record(world, R - 1))]
    assert world.check([world.row(r) for _, r in cases], names=[n for n, _ in cases]) == [ACCEPT] * len(cases)


# ---- forged proofs ---------------------------------------------------------------------------------------------------------------
def test_forged_proofs(world):
    k, rng = world.key, random.Random(0xF0E6)
    a, b = world.recs[0], world.recs[1]
    bump = lambda xs, j: [(x + 1) % R if i == j else x for i, x in enumerate(xs)]
    s = lambda: rng.randrange(1, R)
    eq_only = D.random_record(k, rng, eq_nonce=s())
    h_bit = bytearray(a.h_q)
    h_bit[17] ^= 0x10
    cases = [("pi0.s[0][1] + 1", but(a, pi0_s=bump(a.pi0_s, 1)), (REJECT, ACCEPT)), ("pi0.s[1][1] + 1", but(a, pi0_s=bump(a.pi0_s, 3)), (REJECT, ACCEPT)),
             ("pi1.s[0][0] + 1", but(a, pi1_s=bump(a.pi1_s, 0)), (ACCEPT, REJECT)), ("pi1.s[1][1] + 1", but(a, pi1_s=bump(a.pi1_s, 2)), (ACCEPT, REJECT)),
             ("eq_pos alone", eq_only, (REJECT, ACCEPT)), ("m + 1", but(a, m=(a.m + 1) % R), (ACCEPT, REJECT)),
             ("one bit of h_Q", but(a, h_q=bytes(h_bit)), (ACCEPT, REJECT)), ("com0 of a neighbour", but(a, com0=b.com0), (ACCEPT, REJECT)),
             ("com1 and comz swapped", but(a, com1=a.comz, comz=a.com1), (REJECT, REJECT))]
    # that only eq_pos fails in its case: both challenges are the transcripts' own
    row = world.row(eq_only)
    assert eq_only.pi0_s[0] != eq_only.pi0_s[2]
    assert D.dlog_verify(D.CONTEXT_PI0, eq_only.pi0_c, [eq_only.pi0_s[:2], eq_only.pi0_s[2:]], [[k.gp, k.h], [k.g, k.h]], [eq_only.com1_orig, eq_only.com1])
    rows = [world.row(r) for _, r, _ in cases]
    for (name, _, parts), r in zip(cases, rows):
        assert world.want(r)[:2] == (REJECT, parts), name          # the restatement itself rejects, in the part expected
    honest = world.row(a)
    got = world.check([honest] + rows + [honest], names=["honest"] + [n for n, _, _ in cases] + ["honest"])
    assert got == [ACCEPT] + [REJECT] * len(cases) + [ACCEPT] and row in rows


# ---- malformed rows --------------------------------------------------------------------------------------------------------------
def test_malformed_rows_stay_alone(world):
    a = world.recs[2]
    cases = []
    for f in ("com0", "com1_orig", "com1", "comz"):
        x, y = getattr(a, f)
        off = D.fe(x) + D.fe((y + 1) % Q)
        big = D.fe(Q) + D.fe(y)
        flags = bytearray(o.g1_uncompressed((x, y)))
        flags[63] |= 0xC0
        big_y = bytearray(D.fe(x) + D.fe(Q))
        cases += [(f + " off the curve", but(a, **{f: off})), (f + " with x = q", but(a, **{f: big})), (f + " with y = q", but(a, **{f: bytes(big_y)})),
                  (f + " with both flag bits", but(a, **{f: bytes(flags)}))]
    for f in ("m", "pi0_c", "pi1_c"):
        cases.append((f + " = r", but(a, **{f: R})))
    for j in range(4):
        cases.append(("pi0_s[%d] = r" % j, but(a, pi0_s=[R if i == j else v for i, v in enumerate(a.pi0_s)])))
    for j in range(3):
        cases.append(("pi1_s[%d] = r" % j, but(a, pi1_s=[R if i == j else v for i, v in enumerate(a.pi1_s)])))
    honest = world.row(a)
    rows = []
    for _, r in cases:
        rows += [world.row(r), honest]
    for (name, _), r in zip(cases, rows[::2]):
        assert world.want(r) == (MALFORMED, (MALFORMED, MALFORMED), bytes(32)), name
    got = world.check([honest] + rows, names=["honest"] + [x for n, _ in cases for x in (n, "honest after " + n)])
    assert got == [ACCEPT] + [MALFORMED, ACCEPT] * len(cases)


def test_a_point_at_infinity_with_coordinate_bytes_is_infinity(mdl):
    """ark reads the flag and returns the identity whatever the coordinates hold, as long as they are canonical"""
    rec = steered_records(mdl)[1][1]
    odd = bytearray(D.fe(5) + D.fe(7))
    odd[63] |= 0x40
    row = mdl.row(but(rec, comz=bytes(odd)))
    assert mdl.want(row) == (ACCEPT, (ACCEPT, ACCEPT), rec.digest)
    assert mdl.check([row]) == [ACCEPT]


def test_the_convenience_entry_over_device_link_proofs(mdl):
    cc, k = mdl.cc, mdl.key
    recs = [mdl.recs[0], but(mdl.recs[1], m=(mdl.recs[1].m + 1) % R), mdl.recs[2]]
    rows = [mdl.row(r) for r in recs]
    proofs = [cc.DeviceLinkProof(o.g1_uncompressed(r.com1), o.g1_uncompressed(r.comz), r.h_q, r.m, r.pi0_c, [r.pi0_s[:2], r.pi0_s[2:]], r.pi1_c,
                                 [r.pi1_s[:1], r.pi1_s[1:]]) for r in recs]
    committed = [[row[0][64 * i:64 * i + 64] for i in range(len(k.com))] for row in rows]
    want = [mdl.want(row)[0] == ACCEPT for row in rows]
    assert want == [True, False, True]
    assert cc.Groth16.device_link_verify_batch(mdl.pvk, k.io, k.pos0, k.pos1, committed, proofs) == want


# ---- the call itself -------------------------------------------------------------------------------------------------------------
def test_argument_errors_touch_nothing(mdl):
    from crescent_credentials_amd import api
    L, k = mdl.cc.lib(), mdl.key
    arrays = [np.frombuffer(b, np.uint8).copy() for b in D.pack([mdl.row(mdl.recs[0])])]
    io = np.array(k.io, np.uint8)
    out = [np.full(n, 0xA5, np.uint8) for n in (1, 2, 32)]
    p = lambda a: a.ctypes.data

    def call(io_=io, n_io=len(k.io), pos0=k.pos0, pos1=k.pos1, committed=p(arrays[0]), rows=[p(a) for a in arrays[1:]], h_len=32, n=1, outs=None):
        c_rows = api._CgDeviceLinkRows(*rows)
        o_ = [p(a) for a in out] if outs is None else outs
        rc = L.cg_device_link_verify_batch(mdl.pvk._h, p(io_), n_io, pos0, pos1, committed, ctypes.byref(c_rows), h_len, n, *o_)
        assert all((a == 0xA5).all() for a in out)
        return rc

    assert call(n_io=len(k.io) - 1) == MALFORMED_KEY
    assert call(io_=np.array([2, 1, 2, 3, 0], np.uint8)) == INVALID_ARGUMENT
    for kw in (dict(pos0=5), dict(pos1=5), dict(pos0=1), dict(pos1=4), dict(pos0=3, pos1=3), dict(h_len=65), dict(committed=None),
               dict(outs=[None, p(out[1]), p(out[2])]), dict(outs=[p(out[0]), p(out[1]), None])):
        assert call(**kw) == INVALID_ARGUMENT, kw
    for j in range(8):
        assert call(rows=[None if i == j else p(a) for i, a in enumerate(arrays[1:])]) == INVALID_ARGUMENT, j
    assert call(n=0) == 0
    # part_verdicts may be left out
    rc = L.cg_device_link_verify_batch(mdl.pvk._h, p(io), len(k.io), k.pos0, k.pos1, p(arrays[0]), ctypes.byref(api._CgDeviceLinkRows(*[p(a) for a in arrays[1:]])),
                                       32, 1, p(out[0]), None, p(out[2]))
    assert rc == 0 and out[0][0] == ACCEPT and (out[1] == 0xA5).all() and out[2].tobytes() == mdl.recs[0].digest


def test_the_same_call_again(mdl):
    """the per-call arrays are shared and only grow: a larger and a smaller call in between change nothing.  The same after a
    cg_verify_showings_batch on the handle is tests/test_gpu_showings_device_link.py's: the verifier's pairing kernels declare a
    private segment, which the runtime then keeps for the process, and this file runs in the process, and before the file,
    in which tests/test_gpu_fullsize.py fills the device's memory to a stated remainder."""
    rows = [mdl.row(r) for r in mdl.recs[:5]] + [mdl.row(but(mdl.recs[5], m=R))]
    flat = lambda res: [a.tobytes() for a in res]
    first = flat(mdl.call(rows))
    assert flat(mdl.call(rows)) == first
    mdl.call([mdl.row(mdl.recs[i % 8]) for i in range(200)])
    mdl.call(rows[:1])
    assert flat(mdl.call(rows)) == first
    ms = mdl.pvk.device_link_last_kernel_ms()
    assert len(ms) == 4 and all(t > 0 for t in ms)
