"""Creating showings without a GPU: the three entries are declared, exported, bound and declared to Rust;
cg_show_rand_count and the host-only cg_show_respond_batch (the responses of `DLogPoK::prove`, creds/src/dlog.rs:101-109)
against `show_vectors.make_show`; argument errors of cg_show_commit_batch that are reported before any HIP call; and the
edge vectors tests/test_gpu_show_create.py measures the kernels with, checked here by the oracle alone: each produces the
identity where its name says so, and each is a showing the verifier accepts."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import ark_files
from conftest import ROOT
import show_create_vectors as M
import show_vectors as S

R = M.R
CG_ERR_INVALID_ARGUMENT = -1
ELLS = [1, 2, 6, 26]


def test_entries_are_declared_exported_and_bound(cc):
    from crescent_credentials_amd import api
    hdr = open(os.path.join(ROOT, "include", "crescent_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "sys.rs")).read()
    L = ctypes.CDLL(cc.library_path())
    for name, n_args in (("cg_show_rand_count", 3), ("cg_show_commit_batch", 12), ("cg_show_respond_batch", 8)):
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert hasattr(L, name), name
        assert len(api._SIGNATURES[name][1]) == n_args, name
        assert re.search(r"pub fn %s\s*\(" % name, sys_rs), name
    assert re.search(r"CG_SHOW_MADE = 1, CG_SHOW_MALFORMED = 2", code)
    # the transcript boundary is stated where the entries are declared
    at = hdr.index("cg_show_commit_batch(")
    assert "Merlin" in hdr[hdr.rindex("cg_verify_show_batch(", 0, at):at]
    assert (cc.CG_SHOW_MADE, cc.CG_SHOW_MALFORMED) == (1, 2)
    for f in ("show_commit_batch_packed", "show_respond_batch", "show_batch"):
        assert callable(getattr(cc.Groth16, f))
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "lib.rs")).read()
    assert re.search(r"pub fn show_commit_batch\s*\(", lib_rs) and re.search(r"pub fn show_respond_batch\s*\(", lib_rs)


@pytest.mark.parametrize("ell", ELLS)
@pytest.mark.parametrize("name", M.LAYOUTS)
def test_rand_count(cc, name, ell):
    io = M.layout(name, ell)
    n_com, n_hid, n_resp, n_rand = M.counts(io)
    assert n_resp == 2 * n_com + n_hid + 1 and n_rand == 3 + n_com + n_resp
    assert cc.show_rand_count(io) == n_rand
    arr = (ctypes.c_uint8 * ell)(*io)
    out = ctypes.c_uint64(12345)
    assert cc.lib().cg_show_rand_count(arr, ell, ctypes.byref(out)) == 0 and out.value == n_rand
    arr[ell - 1] = 3
    assert cc.lib().cg_show_rand_count(arr, ell, ctypes.byref(out)) == CG_ERR_INVALID_ARGUMENT and out.value == n_rand
    assert cc.lib().cg_show_rand_count(arr, ell, None) == CG_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def state6():
    rng, sc, vk, xs, abc = M.synthetic(6, 0x5E57)
    return rng, vk, xs, M.proof_of(abc)


def _respond(cc, io, made, cs, status=None, prefill=0):
    _, inputs, rand = M.pack(made)
    n_resp = M.counts(io)[2]
    out = np.full(len(made) * n_resp * 32, prefill, np.uint8)
    arr = np.array(io, np.uint8)
    c = np.frombuffer(M.fe(cs), np.uint8)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    st = None if status is None else np.array(status, np.uint8)
    rc = cc.lib().cg_show_respond_batch(p(arr), arr.size, p(inputs), p(rand), p(c), p(st), len(made), p(out))
    return rc, out.reshape(len(made), n_resp * 32)


@pytest.mark.parametrize("name", M.LAYOUTS)
def test_respond_matches_make_show(cc, state6, name):
    """one showing per challenge of show_vectors.C_VALUES (0, 1, 2^248 - 1, 2^253, r - 1)"""
    rng, vk, xs, proof = state6
    io = M.layout(name, 6)
    made = [M.make(vk, proof, xs, io, rng, c=c) for c in S.C_VALUES]
    want = [M.expected(io, m)[4] for m in made]
    rc, got = _respond(cc, io, made, S.C_VALUES)
    assert rc == 0, cc.lib().cg_last_error()
    for i, w in enumerate(want):
        assert got[i].tobytes() == w, (name, S.C_VALUES[i])
    # and through the package
    _, inputs, rand = M.pack(made)
    s = cc.Groth16.show_respond_batch(io, inputs, rand, list(S.C_VALUES))
    assert s.shape == (len(made), M.counts(io)[2], 32) and s.tobytes() == b"".join(want)
    if name != "mixed":
        return
    # a status that skips one showing: zero bytes there, and that showing is not read (its c is r)
    cs = list(S.C_VALUES)
    cs[1] = R
    rc, got = _respond(cc, io, made, cs, status=[M.MADE, M.MALFORMED, M.MADE, M.MADE, M.MADE], prefill=0xAB)
    assert rc == 0, cc.lib().cg_last_error()
    for i, w in enumerate(want):
        assert got[i].tobytes() == (bytes(len(w)) if i == 1 else w), i
    # r as a nonce, as a read input, as c: an argument error that names the showing and writes nothing
    n_com = M.counts(io)[0]

    def broken(which):
        ms = [M.Made(m.proof, list(m.inputs), list(m.rand), m.show, m.proof_bytes) for m in made]
        cs = list(S.C_VALUES)
        if which == "nonce":
            ms[3].rand[3 + n_com + 2] = R
        elif which == "input":
            ms[3].inputs[io.index(S.HIDDEN)] = R
        else:
            cs[3] = R
        return ms, cs

    for which in ("nonce", "input", "c"):
        ms, cs = broken(which)
        rc, got = _respond(cc, io, ms, cs, prefill=0xAB)
        assert rc == CG_ERR_INVALID_ARGUMENT, which
        assert b"showing 3" in cc.lib().cg_last_error(), which
        assert (got == 0xAB).all(), which
    # r at a revealed position is not read
    ms, cs = broken("c")
    ms[3].inputs[io.index(S.REVEALED)] = R
    rc, got = _respond(cc, io, ms, S.C_VALUES)
    assert rc == 0 and got[3].tobytes() == want[3]


def test_null_handle_is_an_argument_error(cc):
    L = cc.lib()
    io = (ctypes.c_uint8 * 2)(0, 1)
    buf = (ctypes.c_uint8 * 1024)()
    for n in (1, 0):
        assert L.cg_show_commit_batch(None, io, 2, buf, buf, buf, n, buf, buf, buf, buf, buf) == CG_ERR_INVALID_ARGUMENT
        assert b"null" in L.cg_last_error()


def test_edge_vectors_are_what_their_names_say():
    """the oracle alone: which outputs are the identity, and that every edge showing is one the verifier accepts, with the
    k_i the verifier recomputes equal to the prover's"""
    vk, io, cases = M.edge_cases()
    ora = ark_files.prepare_verifying_key(vk)
    assert len(cases) == 15
    for name, m, zero in cases:
        assert M.outputs_that_are_o(m) == zero, name
        assert S.accepts(ora, vk, io, m.show), name
        assert S.recomputed_k(vk, io, m.show) == m.show.k, name
    by = {name.split(":")[0]: m for name, m, _ in cases}
    assert by["proof A = O"].proof[0] is None and by["proof B = O"].proof[1] is None and by["proof C = O"].proof[2] is None
    m = by["every window 0xFF as r_0 and as a nonce"]
    assert m.rand[2] == M.ALL_FF and m.rand.count(M.ALL_FF) == 3 and M.ALL_FF.to_bytes(32, "little") == b"\xff" * 31 + b"\x2f"
