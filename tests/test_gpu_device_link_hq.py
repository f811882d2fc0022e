"""h_Q on the GPU (csrc/devicelinkmake.hip: cg_poseidon_p256_permute_batch, cg_hq_batch, cg_device_link_prove_hq_batch;
csrc/poseidon_p256.hpp, csrc/fp256.hpp): Poseidon of width 3 over P-256's base field and `compute_hQ` on it, alone and in front
of the device-link maker.

Expected bytes come from tests/poseidon_vectors.py, a pure-Python restatement that shares no code with the library, and for
the proofs from tests/device_link_vectors.py fed that h_Q; where Python on every row would take too long, from the g++ build
of the same header (tests/cpp/test_poseidon_p256.cpp), which tests/test_poseidon_p256_host.py holds against Python.  Every
comparison is byte for byte."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import device_link_vectors as D
import poseidon_vectors as PV
import test_gpu_device_link_make as M
from conftest import ROOT

pytestmark = pytest.mark.gpu

P, R = PV.P256, D.R
MADE, MALFORMED_ROW = 1, 2
INVALID_ARGUMENT, MALFORMED_KEY = -1, -6
ACCEPT = D.ACCEPT
fe = D.fe


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


@pytest.fixture(scope="module", params=list(M.T.LAYOUTS))
def world(request, cc):
    w = M.World(cc, request.param, 0x4051 + len(request.param))
    yield w
    w.pvk.close()


@pytest.fixture(scope="module")
def mdl(cc):
    w = M.World(cc, "mdl", 0x4052)
    yield w
    w.pvk.close()


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("poseidon_p256_gpu") / "test_poseidon_p256")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", path, os.path.join(ROOT, "tests", "cpp", "test_poseidon_p256.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def triple(q):
    return b"".join(fe(x) for x in q)


def with_hq(s):
    """a proof's scalars with the h_Q Python computes for them"""
    return dict(s, h_q=PV.hq(s["q0"], s["q1"], s["z"]))


# ---- 1. cg_hq_batch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65])
def test_hq_batch_equals_python(mdl, n):
    rng = random.Random(0x4C0 + n)
    qs = [(1, 2, 3), (0, 0, 0), (R - 1, R - 1, R - 1)][:n] + [tuple(rng.randrange(R) for _ in range(3)) for _ in range(max(n - 3, 0))]
    h, status = mdl.cc.Groth16.hq_batch_packed(mdl.pvk, b"".join(triple(q) for q in qs))
    assert status.tolist() == [MADE] * n
    for i, q in enumerate(qs):
        assert h[i].tobytes() == PV.hq(*q), i
    assert h[0].tobytes().hex() == "b4c83f5ebbc2a8a6c913d1361168ceee2d3796453258470cb7ac7c3abeb24ab5"


# ---- 2. across a chunk ----------------------------------------------------------------------------------------------------------
def test_hq_batch_across_a_chunk_with_malformed_rows_at_its_edges(mdl, host_exe, tmp_path):
    """997 distinct triples tiled over chunk + 1 rows, so that the host program answers every row in a fraction of a second"""
    chunk = M.chunk_size()
    assert chunk == 1 << 15
    n, distinct = chunk + 1, 997
    at = (0, chunk - 1, chunk)
    rng = random.Random(0xC4A2)
    base = np.frombuffer(b"".join(triple([rng.randrange(R) for _ in range(3)]) for _ in range(distinct)), np.uint8).reshape(distinct, 96)
    q = base[np.arange(n) % distinct].copy()
    for i, bad in zip(at, ((R, 1, 1), (1, (1 << 256) - 1, 1), (1, 1, R))):
        q[i] = np.frombuffer(triple(bad), np.uint8)
    h, status = mdl.cc.Groth16.hq_batch_packed(mdl.pvk, q.reshape(-1))
    # every row against the host build of the header
    src, dst = str(tmp_path / "q.bin"), str(tmp_path / "h.bin")
    base.tofile(src)
    r = subprocess.run([host_exe], input="hqfile %s %s %d\n" % (src, dst, distinct), capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == [str(distinct)], r.stdout + r.stderr
    raw = np.fromfile(dst, np.uint8)
    host_h, host_status = raw[:32 * distinct].reshape(distinct, 32), raw[32 * distinct:]
    assert (host_status == MADE).all()
    want = host_h[np.arange(n) % distinct].copy()
    want[list(at)] = 0
    assert np.array_equal(h, want)
    assert (status == MADE).sum() == n - 3 and (status[list(at)] == MALFORMED_ROW).all()
    # the edge rows' neighbours and 64 random rows against Python
    rows = sorted({1, chunk - 2, chunk - 3, 2} | set(rng.sample(range(n), 64)) - set(at))
    assert len(rows) >= 64
    for i in rows:
        vals = [int.from_bytes(q[i, 32 * j:32 * j + 32].tobytes(), "little") for j in range(3)]
        assert h[i].tobytes() == PV.hq(*vals), i


# ---- 3. the permutation at the field's edges ---------------------------------------------------------------------------------------
def test_permute_batch_at_the_fields_edges(mdl):
    c = PV.p256()
    rng = random.Random(0x9E12)
    states = [[0, 0, 0], [P - 1, P - 1, P - 1]]
    for v in (0, 1, P - 1):                                        # the first round's S-box inputs: state + rc[0..3)
        states.append([(v - c.rc[i]) % P for i in range(3)])
    assert [(x + k) % P for x, k in zip(states[4], c.rc[:3])] == [P - 1] * 3
    states += [[rng.randrange(P) for _ in range(3)] for _ in range(64)]
    bad = {7: [P, 0, 0], 8: [5, (1 << 256) - 1, 6], 40: [1, 2, P], 41: [(1 << 256) - 1] * 3}
    for i, st in bad.items():
        states.insert(i, st)
    out, status = mdl.cc.Groth16.poseidon_p256_permute_batch_packed(mdl.pvk, b"".join(triple(st) for st in states))
    assert len(states) == 73
    for i, st in enumerate(states):
        if i in bad:
            assert status[i] == MALFORMED_ROW and not out[i].any(), i
        else:
            assert status[i] == MADE and out[i].tobytes() == triple(PV.permute(c, st)), i


# ---- 4. h_Q in front of the maker ---------------------------------------------------------------------------------------------------
def test_prove_hq_batch_equals_the_two_calls_and_python(world):
    k, G = world.key, world.cc.Groth16
    secrets = [with_hq(s) for s in world.secrets]
    cases = [secrets[i % 8] for i in range(65)]
    rows = [world.row(s) for s in cases]
    wrong = world.row(secrets[2], q0=(secrets[2]["q0"] + 1) % R)   # an opening that does not open com0
    rows[33] = wrong
    ins = [b"".join(r[j] for r in rows) for j in range(3)]
    got = G.device_link_prove_hq_batch_packed(world.pvk, k.io, k.pos0, k.pos1, *ins)
    assert len(got) == 10
    # the two calls
    q = b"".join(r[1][0:32] + r[1][64:96] + r[2][0:32] for r in rows)
    h, h_status = G.hq_batch_packed(world.pvk, q)
    assert h_status.tolist() == [MADE] * 65
    two = G.device_link_prove_batch_packed(world.pvk, k.io, k.pos0, k.pos1, *ins, h.reshape(-1), h_len=32)
    for j in range(9):
        assert np.array_equal(got[j], two[j]), j
    h_want = h.copy()
    h_want[33] = 0
    assert np.array_equal(got[9], h_want)
    # Python: the restatement's prover fed the restatement's h_Q
    for i, s in enumerate(cases):
        row = tuple(a[i].tobytes() for a in got)
        if i == 33:
            assert row == M.ZERO_ROW + (bytes(32),)
        else:
            assert row == world.want(s) + (s["h_q"],), i
    assert got[8][33] == MALFORMED_ROW and (np.delete(got[8], 33) == MADE).all()
    # and the verifier takes them with the h_Q the call returned
    keep = [i for i in range(65) if i != 33]
    com1, comz, m, c0, s0, c1, s1, e, _, hq = [a[keep] for a in got]
    verdicts, _, e2 = G.device_link_verify_batch_packed(world.pvk, k.io, k.pos0, k.pos1, b"".join(rows[i][0] for i in keep), com1, comz, hq.reshape(-1),
                                                        m, c0, s0, c1, s1, h_len=32)
    assert verdicts.tolist() == [ACCEPT] * 64 and np.array_equal(e2, e)


def test_the_convenience_entry_returns_proofs_with_their_hq(mdl):
    cc, k = mdl.cc, mdl.key
    ss = [with_hq(s) for s in mdl.secrets[:3]]
    committed = [[mdl.row(s)[0][64 * i:64 * i + 64] for i in range(len(k.com))] for s in ss]
    openings = [[s[f] for f in M.OPEN] for s in ss]
    openings[1][0] = (openings[1][0] + 1) % R
    proofs, digests = cc.Groth16.device_link_prove_hq_batch(mdl.pvk, k.io, k.pos0, k.pos1, committed, openings, rand=[[s[f] for f in M.RAND] for s in ss])
    assert proofs[1] is None and not digests[1].any()
    for i in (0, 2):
        assert proofs[i].h_q == ss[i]["h_q"] and digests[i].tobytes() == mdl.rec(ss[i]).digest
    assert cc.Groth16.device_link_verify_batch(mdl.pvk, k.io, k.pos0, k.pos1, [committed[0], committed[2]], [proofs[0], proofs[2]]) == [True, True]


# ---- 5. argument errors -----------------------------------------------------------------------------------------------------------
def test_argument_errors_touch_nothing(mdl):
    from crescent_credentials_amd import api
    L, k = mdl.cc.lib(), mdl.key
    ins = [np.frombuffer(b, np.uint8).copy() for b in mdl.row(mdl.secrets[0])[:3]]
    io = np.array(k.io, np.uint8)
    out = [np.full(n, 0xA5, np.uint8) for n in M.WIDTHS + (32,)]
    p = lambda a: a.ctypes.data

    def call(io_=io, n_io=len(k.io), pos0=k.pos0, pos1=k.pos1, arrays=[p(a) for a in ins], n=1, rows=[p(a) for a in out[:7]], e=p(out[7]),
             status=p(out[8]), h_q=p(out[9]), made="struct"):
        c_made = api._CgDeviceLinkMade(*rows)
        rc = L.cg_device_link_prove_hq_batch(mdl.pvk._h, p(io_), n_io, pos0, pos1, *arrays, n, ctypes.byref(c_made) if made == "struct" else None, e,
                                             status, h_q)
        assert all((a == 0xA5).all() for a in out)
        return rc

    assert call(n_io=len(k.io) - 1) == MALFORMED_KEY
    assert call(io_=np.array([2, 1, 2, 3, 0], np.uint8)) == INVALID_ARGUMENT
    for kw in (dict(pos0=5), dict(pos1=5), dict(pos0=1), dict(pos1=4), dict(pos0=3, pos1=3), dict(made=None), dict(e=None), dict(status=None),
               dict(h_q=None)):
        assert call(**kw) == INVALID_ARGUMENT, kw
        assert kw != dict(h_q=None) or b"null" in L.cg_last_error()
    for j in range(3):
        assert call(arrays=[None if i == j else p(a) for i, a in enumerate(ins)]) == INVALID_ARGUMENT, j
    for j in range(7):
        assert call(rows=[None if i == j else p(a) for i, a in enumerate(out[:7])]) == INVALID_ARGUMENT, j
    assert call(n=0) == 0
    # the two plain entries
    q = np.frombuffer(triple((1, 2, 3)), np.uint8).copy()
    big, status = np.full(96, 0xA5, np.uint8), np.full(1, 0xA5, np.uint8)
    for fn in (L.cg_hq_batch, L.cg_poseidon_p256_permute_batch):
        for args in ((None, p(big), p(status)), (p(q), None, p(status)), (p(q), p(big), None)):
            assert fn(mdl.pvk._h, args[0], 1, args[1], args[2]) == INVALID_ARGUMENT and b"null" in L.cg_last_error()
        assert fn(mdl.pvk._h, None, 0, None, None) == 0
        assert (big == 0xA5).all() and (status == 0xA5).all()


# ---- 6. the handle's state ------------------------------------------------------------------------------------------------------------
def test_the_same_call_again_and_beside_the_other_entries(cc):
    """the constants go up once, and the h_Q arrays, the maker's and the verifier's do not evict each other"""
    w = M.World(cc, "mdl", 0x4056)
    try:
        k, G = w.key, cc.Groth16
        assert w.pvk.hq_last_kernel_ms() == (0.0, 0.0, 0)
        secrets = [with_hq(s) for s in w.secrets[:5]]
        rows = [w.row(s) for s in secrets]
        ins = [b"".join(r[j] for r in rows) for j in range(3)]
        as_bytes = lambda out: [a.tobytes() for a in out]
        first = as_bytes(G.device_link_prove_hq_batch_packed(w.pvk, k.io, k.pos0, k.pos1, *ins))
        assert first[9] == b"".join(s["h_q"] for s in secrets)
        t_hash, t_link, uploads = w.pvk.hq_last_kernel_ms()
        assert t_hash == 0.0 and t_link > 0 and uploads == 1
        assert as_bytes(G.device_link_prove_hq_batch_packed(w.pvk, k.io, k.pos0, k.pos1, *ins)) == first
        # a verifying call, a larger h_Q call and a plain proving call in between
        verdicts, _ = w.verify(rows, [np.frombuffer(b, np.uint8) for b in first[:9]])
        assert verdicts.tolist() == [ACCEPT] * 5
        rng = random.Random(0x57A7)
        many = [tuple(rng.randrange(R) for _ in range(3)) for _ in range(200)]
        h, _ = G.hq_batch_packed(w.pvk, b"".join(triple(q) for q in many))
        assert h[199].tobytes() == PV.hq(*many[199]) and h[0].tobytes() == PV.hq(*many[0])
        assert [tuple(a[i].tobytes() for a in w.call(rows)) for i in range(5)] == [w.want(s) for s in secrets]
        assert as_bytes(G.device_link_prove_hq_batch_packed(w.pvk, k.io, k.pos0, k.pos1, *ins)) == first
        t_hash, t_link, uploads = w.pvk.hq_last_kernel_ms()
        assert t_hash > 0 and t_link > 0 and uploads == 1
        ms = w.pvk.device_link_prove_last_kernel_ms()
        assert len(ms) == 6 and all(t > 0 for t in ms)
    finally:
        w.pvk.close()
