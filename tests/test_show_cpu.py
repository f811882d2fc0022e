"""Showings without a GPU: the vectors of tests/show_vectors.py satisfy `verify_proof_with_prepared_inputs` under the
oracle's pairing (and stop doing so when a revealed input changes) - which guards the yardstick tests/test_gpu_show.py
measures cg_verify_show_batch with - the ShowGroth16 byte layout of the package against an independent writer, and the
host side of the new entry: declared, exported, bound, and argument errors reported before any HIP call."""
import ctypes
import os
import random
import re

import pytest

import ark_files
import bn254_oracle as o
from conftest import ROOT
import show_vectors as S
import verify_vectors as V

R = o.R
CG_ERR_INVALID_ARGUMENT = -1


def _synthetic(ell, seed):
    """a gamma = 1 key from chosen scalars, inputs, and an accepting proof"""
    rng = random.Random(seed)
    alpha, beta, delta = (rng.randrange(1, R) for _ in range(3))
    sc = (alpha, beta, 1, delta, [rng.randrange(R) for _ in range(ell + 1)])
    xs = [rng.randrange(R) for _ in range(ell)]
    proof = V.synthetic_proof(sc, xs, a=rng.randrange(1, R), b=rng.randrange(1, R))
    return rng, sc, V.synthetic_vk(*sc[:4], sc[4]), xs, proof


@pytest.mark.parametrize("layout", ["mixed", "all_hidden"])
def test_helper_showings_satisfy_the_pairing_equation(layout):
    rng, sc, vk, xs, proof = _synthetic(5, 41)
    io = S.jwt_like_layout(5) if layout == "mixed" else [S.HIDDEN] * 5
    sh = S.make_show(vk, proof, xs, io, rng)
    assert S.pairing_accepts(vk, io, sh)
    assert S.accepts(ark_files.prepare_verifying_key(vk), vk, io, sh)
    assert S.recomputed_k(vk, io, sh) == sh.k
    assert len(sh.s) == io.count(S.COMMITTED) + 1 and sum(len(si) for si in sh.s) == 2 * io.count(S.COMMITTED) + io.count(S.HIDDEN) + 1


def test_a_changed_revealed_input_breaks_the_equation():
    rng, sc, vk, xs, proof = _synthetic(5, 43)
    io = S.jwt_like_layout(5)
    sh = S.make_show(vk, proof, xs, io, rng)
    assert sh.revealed
    sh.revealed[0] = (sh.revealed[0] + 1) % R
    assert not S.pairing_accepts(vk, io, sh)
    assert not S.accepts(ark_files.prepare_verifying_key(vk), vk, io, sh)


def test_golden_key_showing_accepts():
    pk, _, w, g = V.golden_vk("d8")
    vk = pk["vk"]
    xs = w[1:g["num_inputs"]]
    proof_b = bytes.fromhex(g["proofs"][0]["proof"])
    rd = ark_files._Rd(proof_b)
    proof = (rd.g1(), rd.g2(), rd.g1())
    io = S.jwt_like_layout(len(xs))
    sh = S.make_show(vk, proof, xs, io, random.Random(3))
    assert S.accepts(ark_files.prepare_verifying_key(vk), vk, io, sh)


def test_show_groth16_ark_bytes_roundtrip(cc):
    rng, sc, vk, xs, proof = _synthetic(6, 47)
    for io in (S.jwt_like_layout(6), [S.REVEALED] * 6, [S.COMMITTED] * 6):
        sh = S.make_show(vk, proof, xs, io, rng)
        want = S.ark_bytes(sh)
        mine, _ = S.api_show(cc, sh)
        assert mine.to_ark_bytes() == want
        back = cc.ShowGroth16.from_ark_bytes(want)
        assert back == mine and back.to_ark_bytes() == want
        assert len(want) == 256 + 64 + 32 + 8 + sum(8 + 32 * len(si) for si in sh.s) + 8 + 64 * len(sh.committed)
        for bad in (want[:-1], want + b"\0", want[:300]):
            with pytest.raises(ValueError):
                cc.ShowGroth16.from_ark_bytes(bad)


def test_entry_is_declared_exported_and_bound(cc):
    from crescent_credentials_amd import api
    hdr = open(os.path.join(ROOT, "include", "crescent_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+cg_verify_show_batch\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m and len(m.group(1).split(",")) == 12
    assert re.search(r"CG_IO_REVEALED = 0, CG_IO_HIDDEN = 1, CG_IO_COMMITTED = 2", code)
    assert "Merlin" in hdr                                   # the transcript boundary is stated where the entry is declared
    assert hasattr(ctypes.CDLL(cc.library_path()), "cg_verify_show_batch")
    assert len(api._SIGNATURES["cg_verify_show_batch"][1]) == 12
    assert (cc.CG_IO_REVEALED, cc.CG_IO_HIDDEN, cc.CG_IO_COMMITTED) == (0, 1, 2)
    assert callable(cc.Groth16.verify_show_batch)
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "sys.rs")).read()
    assert re.search(r"pub fn cg_verify_show_batch\s*\(", sys_rs)


def test_null_handle_is_an_argument_error(cc):
    L = cc.lib()
    io = (ctypes.c_uint8 * 2)(0, 1)
    buf = (ctypes.c_uint8 * 256)()
    assert L.cg_verify_show_batch(None, io, 2, buf, buf, buf, buf, None, None, 1, buf, None) == CG_ERR_INVALID_ARGUMENT
    assert L.cg_verify_show_batch(None, io, 2, buf, buf, buf, buf, None, None, 0, buf, None) == CG_ERR_INVALID_ARGUMENT
    assert b"null" in L.cg_last_error()
