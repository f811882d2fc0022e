"""The BN254 half of device proofs MADE on the GPU (csrc/devicelinkmake.hip: cg_device_link_prove_batch;
csrc/device_link_make.hpp): `DeviceProof::prove` (creds/src/device.rs:104-160) short of `compute_hQ` and pi2, for batches of
device-bound showings.

Every expected byte comes from tests/device_link_vectors.py (`prove`, `record_bytes`), a pure-Python restatement that shares no
code with the library; every comparison is byte for byte.  What the call makes is also handed to cg_device_link_verify_batch.
The two layouts of tests/test_gpu_device_link.py, so that the committed indices are derived and not assumed.  The case that goes
through cg_create_showings_batch lives in tests/test_gpu_showings_device_link_make.py, for the reason
tests/test_gpu_showings_device_link.py states.

On the coincident sums: the prover's sums are of two walks each, s·base + t·h, and the key's discrete logarithms are known, so
t is chosen to make the two partials EQUAL (the general addition has to double) or OPPOSITE (the sum is O, whose text form is
"infinity" and whose compressed form is the flag alone)."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import device_link_vectors as D
import test_gpu_device_link as T
from conftest import ROOT

pytestmark = pytest.mark.gpu

o = D.o
R, Q = D.R, D.Q
MADE, NOT_MADE = 1, 2
ACCEPT, MALFORMED = D.ACCEPT, D.MALFORMED
INVALID_ARGUMENT, MALFORMED_KEY = -1, -6
OPEN = ("q0", "r0", "q1", "r1_orig")
RAND = ("z", "tz", "r1", "a", "b", "d", "n0", "n1", "n2")
WIDTHS = (64, 64, 32, 32, 128, 32, 96, 32, 1)                     # com1, comz, m, pi0_c, pi0_s, pi1_c, pi1_s, e_out, status
ZERO_ROW = tuple(bytes(n) for n in WIDTHS[:-1]) + (bytes([NOT_MADE]),)
inv = T.inv
fe = D.fe


def chunk_size():
    src = open(os.path.join(ROOT, "crescent-credentials_amd", "csrc", "devicelinkmake.hip")).read()
    return eval(re.search(r"constexpr uint64_t DLMCHUNK = ([0-9u<> ]+);", src).group(1).replace("u", ""))


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


def scalars(rng, h_len=32, **kw):
    """the 13 scalars and h_Q of one proof, by name"""
    s = {f: rng.randrange(1, R) for f in OPEN + RAND}
    s["h_q"] = bytes(rng.randrange(256) for _ in range(h_len))
    s.update(kw)
    return s


class World:
    """one synthetic key under a layout, loaded on the GPU, with eight honest sets of scalars; the restatement's proofs cached"""

    def __init__(self, cc, name, seed):
        io, pos0, pos1 = T.LAYOUTS[name]
        self.cc, self.key = cc, D.make_key(io, pos0, pos1, seed)
        self.pvk = cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(T.V.vk_bytes(self.key.vk)))
        self.rng = random.Random(seed ^ 0x3A4E)
        self.secrets = [scalars(self.rng) for _ in range(8)]
        self._recs = {}

    def rec(self, s):
        k = tuple(s[f] for f in OPEN + RAND) + (s["h_q"],)
        if k not in self._recs:
            self._recs[k] = D.prove(self.key, s["q0"], s["r0"], s["q1"], s["r1_orig"], s["r1"], s["z"], s["tz"], (s["a"], s["b"], s["d"]),
                                    (s["n0"], s["n1"], s["n2"]), s["h_q"])
        return self._recs[k]

    def row(self, s, **over):
        """one row of the call's four input arrays: (committed, openings, rand, h_q).  The committed points are those the
        scalars s open; `over` replaces a scalar (an int, R and above included) or com0 / com1_orig (bytes) afterwards"""
        rec = self.rec(s)
        committed = D.record_bytes(self.key, T.but(rec, **{f: over[f] for f in ("com0", "com1_orig") if f in over}))[0]
        v = dict(s, **{f: x for f, x in over.items() if f in OPEN + RAND})
        return committed, b"".join(fe(v[f]) for f in OPEN), b"".join(fe(v[f]) for f in RAND), s["h_q"]

    def want(self, s):
        """the row of every output for the scalars s"""
        r, pt = self.rec(s), o.g1_uncompressed
        return (pt(r.com1), pt(r.comz), fe(r.m), fe(r.pi0_c), b"".join(fe(x) for x in r.pi0_s), fe(r.pi1_c), b"".join(fe(x) for x in r.pi1_s),
                r.digest, bytes([MADE]))

    def call(self, rows, h_len=32):
        """-> the nine output arrays"""
        k = self.key
        return self.cc.Groth16.device_link_prove_batch_packed(self.pvk, k.io, k.pos0, k.pos1, *[b"".join(r[j] for r in rows) for j in range(4)],
                                                              h_len=h_len)

    def made(self, rows, h_len=32):
        """-> per row the tuple of its nine output rows as bytes"""
        out = self.call(rows, h_len)
        return [tuple(a[i].tobytes() for a in out) for i in range(len(rows))]

    def verify(self, rows, out, h_len=32):
        """cg_device_link_verify_batch on the rows the maker wrote -> verdicts"""
        k = self.key
        com1, comz, m, c0, s0, c1, s1, _, _ = out
        verdicts, _, e = self.cc.Groth16.device_link_verify_batch_packed(self.pvk, k.io, k.pos0, k.pos1, b"".join(r[0] for r in rows), com1, comz,
                                                                         b"".join(r[3] for r in rows), m, c0, s0, c1, s1, h_len=h_len)
        return verdicts, e

    def check(self, cases, h_len=32):
        """cases: (name, scalars).  Every output row equals the restatement's, and the GPU verifier accepts them all."""
        rows = [self.row(s) for _, s in cases]
        out = self.call(rows, h_len)
        for i, (name, s) in enumerate(cases):
            got, want = tuple(a[i].tobytes() for a in out), self.want(s)
            for j, (g, w_) in enumerate(zip(got, want)):
                assert g == w_, (name, j)
        verdicts, e = self.verify(rows, out, h_len)
        assert verdicts.tolist() == [ACCEPT] * len(cases), [n for (n, _), v in zip(cases, verdicts) if v != ACCEPT]
        assert e.tobytes() == out[7].tobytes()


@pytest.fixture(scope="module", params=list(T.LAYOUTS))
def world(request, cc):
    w = World(cc, request.param, 0xDE71CE + len(request.param))
    yield w
    w.pvk.close()


@pytest.fixture(scope="module")
def mdl(cc):
    w = World(cc, "mdl", 0x3D1)
    yield w
    w.pvk.close()


# ---- honest proofs ---------------------------------------------------------------------------------------------------------------
def test_one_proof(world):
    world.check([("one", world.secrets[0])])
    assert [len(x) for x in world.want(world.secrets[0])] == list(WIDTHS)


def test_a_wave_and_one_lane(world):
    world.check([(i, world.secrets[i % 8]) for i in range(65)])


def test_more_than_a_chunk_with_malformed_rows_at_its_edges(mdl):
    chunk = chunk_size()
    assert chunk == 1 << 15
    n = chunk + 1
    at = (0, chunk - 1, chunk)
    s = mdl.secrets[3]
    off = D.fe(mdl.rec(s).com0[0]) + D.fe((mdl.rec(s).com0[1] + 1) % Q)
    bad = [mdl.row(s, n2=R), mdl.row(s, q0=(s["q0"] + 1) % R), mdl.row(s, com0=off)]       # found by the checks, by the sums, by the checks
    rows = [mdl.row(x) for x in mdl.secrets]
    idx = np.arange(n) % 8
    arrays = [np.stack([np.frombuffer(r[j], np.uint8) for r in rows])[idx].copy() for j in range(4)]
    for i, b in zip(at, bad):
        for j in range(4):
            arrays[j][i] = np.frombuffer(b[j], np.uint8)
    k = mdl.key
    out = mdl.cc.Groth16.device_link_prove_batch_packed(mdl.pvk, k.io, k.pos0, k.pos1, *[a.reshape(-1) for a in arrays], h_len=32)
    want = [mdl.want(x) for x in mdl.secrets]
    for j, width in enumerate(WIDTHS):
        tiled = np.stack([np.frombuffer(w_[j], np.uint8) for w_ in want])[idx].copy()
        for i in at:
            tiled[i] = np.frombuffer(ZERO_ROW[j], np.uint8)
        assert np.array_equal(out[j].reshape(n, width), tiled), j
    com1, comz, m, c0, s0, c1, s1, _, status = out
    assert (status == MADE).sum() == n - 3
    verdicts, _, _ = mdl.cc.Groth16.device_link_verify_batch_packed(mdl.pvk, k.io, k.pos0, k.pos1, arrays[0].reshape(-1), com1, comz, arrays[3].reshape(-1),
                                                                   m, c0, s0, c1, s1, h_len=32)
    accepted = verdicts == ACCEPT
    assert accepted.sum() == n - 3 and not accepted[list(at)].any()
    assert (verdicts[list(at)] == MALFORMED).all()               # a row of zero bytes holds no curve point


# ---- the digest -------------------------------------------------------------------------------------------------------------------
def test_digest_at_every_padding_boundary(mdl):
    """one proof's scalars under h_Q of the lengths that put the message's end at 55, 56, 63, 0 and 1 mod 64"""
    rng = random.Random(0x9AD)
    s = scalars(rng, h_len=0)
    first = mdl.rec(s)
    base = len(D.message(first.pi0_c, first.com0, first.com1, first.comz, b""))
    seen = set()
    for want_mod in (55, 56, 63, 0, 1):
        h_len = (want_mod - base) % 64
        t = dict(s, h_q=bytes(rng.randrange(256) for _ in range(h_len)))
        rec = mdl.rec(t)
        assert len(D.message(rec.pi0_c, rec.com0, rec.com1, rec.comz, rec.h_q)) % 64 == want_mod and 0 <= h_len <= 64
        mdl.check([("end at %d" % want_mod, t)] * 2, h_len=h_len)
        seen.add(want_mod)
    assert len(seen) == 5


# ---- coincident and cancelling sums ----------------------------------------------------------------------------------------------
def test_coincident_and_cancelling_sums(world):
    k, rng = world.key, random.Random(0xCA9C)
    # (the sum, the scalar on g or g', that base's logarithm, the scalar on h)
    pairs = [("comz", "z", k.kg, "tz"), ("com1", "q1", k.kg, "r1"), ("pi0 k_0", "a", k.kgp, "b"), ("pi0 k_1", "a", k.kg, "d"),
             ("pi1 k_1", "n1", k.kg, "n2"), ("opening of com0", "q0", k.kg, "r0"), ("opening of com1_orig", "q1", k.kgp, "r1_orig")]
    cases = []
    for name, f, log, on_h in pairs:
        for kind, sign in (("equal", 1), ("opposite", -1)):
            s = scalars(rng)
            s[on_h] = sign * s[f] * log * inv(k.kh) % R
            assert D.mul(k.h, s[on_h]) == D.mul(o.G1_GEN, sign * s[f] * log % R)
            cases.append(("%s: %s partials" % (name, kind), s))
    by = dict(cases)
    assert world.rec(by["comz: opposite partials"]).comz is None and world.rec(by["com1: opposite partials"]).com1 is None
    assert world.rec(by["opening of com0: opposite partials"]).com0 is None and world.rec(by["opening of com1_orig: opposite partials"]).com1_orig is None
    assert world.rec(by["comz: equal partials"]).comz == D.mul(k.g, 2 * by["comz: equal partials"]["z"])
    cases.append(("every nonce zero", scalars(rng, a=0, b=0, d=0, n0=0, n1=0, n2=0)))
    s = scalars(rng, r0=0, r1=0, tz=0)
    rec = world.rec(s)
    e1, e2 = D.e_of(rec.digest)
    assert D.add(D.add(rec.com0, D.mul(rec.com1, e1)), D.mul(rec.comz, e2)) == D.mul(k.g, rec.m)     # lhs1 = O
    cases.append(("lhs1 = O", s))
    cases.append(("every scalar zero", scalars(rng, **{f: 0 for f in OPEN + RAND})))
    world.check(cases)


# ---- malformed rows --------------------------------------------------------------------------------------------------------------
def test_malformed_rows_stay_alone(world):
    s = world.secrets[2]
    rec = world.rec(s)
    x, y = rec.com0
    flags = bytearray(o.g1_uncompressed(rec.com1_orig))
    flags[63] |= 0xC0
    cases = [(f + " = r", {f: R}) for f in OPEN + RAND]
    cases += [("com0 off the curve", dict(com0=D.fe(x) + D.fe((y + 1) % Q))), ("com1_orig with both flag bits", dict(com1_orig=bytes(flags))),
              ("q0 + 1 against an honest com0", dict(q0=(s["q0"] + 1) % R)), ("r1_orig + 1 against an honest com1_orig", dict(r1_orig=(s["r1_orig"] + 1) % R))]
    assert len(cases) == 13 + 4
    honest = world.row(s)
    rows = [honest]
    for _, over in cases:
        rows += [world.row(s, **over), honest]
    got = world.made(rows)
    alone = world.made([honest])[0]
    assert alone == world.want(s)
    for i, (name, _) in enumerate(cases):
        assert got[1 + 2 * i] == ZERO_ROW, name
        assert got[2 + 2 * i] == alone, "honest after " + name
    assert got[0] == alone


def test_a_committed_point_at_infinity_with_coordinate_bytes_is_infinity(mdl):
    """ark reads the flag and returns the identity whatever the coordinates hold, as long as they are canonical; the digest
    says "infinity" for it"""
    s = scalars(random.Random(0x1F), q0=0, r0=0)
    assert mdl.rec(s).com0 is None
    odd = bytearray(D.fe(5) + D.fe(7))
    odd[63] |= 0x40
    assert mdl.made([mdl.row(s, com0=bytes(odd))]) == [mdl.want(s)]


def test_the_convenience_entry_makes_what_the_verifying_one_takes(mdl):
    cc, k = mdl.cc, mdl.key
    ss = mdl.secrets[:3]
    committed = [[mdl.row(s)[0][64 * i:64 * i + 64] for i in range(len(k.com))] for s in ss]
    openings = [[s[f] for f in OPEN] for s in ss]
    openings[1][0] = (openings[1][0] + 1) % R
    proofs, digests = cc.Groth16.device_link_prove_batch(mdl.pvk, k.io, k.pos0, k.pos1, committed, openings, [s["h_q"] for s in ss],
                                                         rand=[[s[f] for f in RAND] for s in ss])
    assert proofs[1] is None and not digests[1].any()
    for i in (0, 2):
        r = mdl.rec(ss[i])
        assert proofs[i] == cc.DeviceLinkProof(o.g1_uncompressed(r.com1), o.g1_uncompressed(r.comz), r.h_q, r.m, r.pi0_c, [r.pi0_s[:2], r.pi0_s[2:]],
                                               r.pi1_c, [r.pi1_s[:1], r.pi1_s[1:]])
        assert digests[i].tobytes() == r.digest
    assert cc.Groth16.device_link_verify_batch(mdl.pvk, k.io, k.pos0, k.pos1, [committed[0], committed[2]], [proofs[0], proofs[2]]) == [True, True]
    drawn, _ = cc.Groth16.device_link_prove_batch(mdl.pvk, k.io, k.pos0, k.pos1, committed[:1], [[ss[0][f] for f in OPEN]], [ss[0]["h_q"]])
    assert cc.Groth16.device_link_verify_batch(mdl.pvk, k.io, k.pos0, k.pos1, committed[:1], drawn) == [True]


# ---- the call itself -------------------------------------------------------------------------------------------------------------
def test_argument_errors_touch_nothing(mdl):
    from crescent_credentials_amd import api
    L, k = mdl.cc.lib(), mdl.key
    ins = [np.frombuffer(b, np.uint8).copy() for b in mdl.row(mdl.secrets[0])]
    io = np.array(k.io, np.uint8)
    out = [np.full(n, 0xA5, np.uint8) for n in WIDTHS]
    p = lambda a: a.ctypes.data

    def call(io_=io, n_io=len(k.io), pos0=k.pos0, pos1=k.pos1, arrays=[p(a) for a in ins], h_len=32, n=1, rows=[p(a) for a in out[:7]], e=p(out[7]),
             status=p(out[8]), made="struct"):
        c_made = api._CgDeviceLinkMade(*rows)
        rc = L.cg_device_link_prove_batch(mdl.pvk._h, p(io_), n_io, pos0, pos1, *arrays, h_len, n, ctypes.byref(c_made) if made == "struct" else None, e,
                                          status)
        assert all((a == 0xA5).all() for a in out)
        return rc

    assert call(n_io=len(k.io) - 1) == MALFORMED_KEY
    assert call(io_=np.array([2, 1, 2, 3, 0], np.uint8)) == INVALID_ARGUMENT
    for kw in (dict(pos0=5), dict(pos1=5), dict(pos0=1), dict(pos1=4), dict(pos0=3, pos1=3), dict(h_len=65), dict(made=None), dict(e=None),
               dict(status=None)):
        assert call(**kw) == INVALID_ARGUMENT, kw
    for j in range(4):                                             # committed, openings, rand, h_q (with h_len = 32)
        assert call(arrays=[None if i == j else p(a) for i, a in enumerate(ins)]) == INVALID_ARGUMENT, j
    for j in range(7):
        assert call(rows=[None if i == j else p(a) for i, a in enumerate(out[:7])]) == INVALID_ARGUMENT, j
    assert call(n=0) == 0
    # h_q may be left out with h_len = 0
    s = dict(mdl.secrets[0], h_q=b"")
    ins0 = [np.frombuffer(b, np.uint8).copy() for b in mdl.row(s)[:3]]
    c_made = api._CgDeviceLinkMade(*[p(a) for a in out[:7]])
    rc = L.cg_device_link_prove_batch(mdl.pvk._h, p(io), len(k.io), k.pos0, k.pos1, *[p(a) for a in ins0], None, 0, 1, ctypes.byref(c_made), p(out[7]),
                                      p(out[8]))
    assert rc == 0 and tuple(a.tobytes() for a in out) == mdl.want(s)


def test_the_same_call_again(mdl):
    """the per-call arrays are the maker's own and only grow: a larger and a smaller call, and a verifier call on the same
    handle, in between change nothing"""
    s5 = mdl.secrets[5]
    rows = [mdl.row(s) for s in mdl.secrets[:5]] + [mdl.row(s5, z=R)]
    first = mdl.made(rows)
    assert first == [mdl.want(s) for s in mdl.secrets[:5]] + [ZERO_ROW]
    assert mdl.made(rows) == first
    big = [mdl.row(mdl.secrets[i % 8]) for i in range(200)]
    out = mdl.call(big)
    verdicts, _ = mdl.verify(big, out)
    assert verdicts.tolist() == [ACCEPT] * 200
    mdl.call(rows[:1])
    assert mdl.made(rows) == first
    ms = mdl.pvk.device_link_prove_last_kernel_ms()
    assert len(ms) == 6 and all(t > 0 for t in ms)
    assert all(t > 0 for t in mdl.pvk.device_link_last_kernel_ms())
