"""Host side of Groth16 verification (csrc/verify.hip): cg_prepare_verifying_key against the oracle's pvk bytes
(ark_files.pvk_bytes(prepare_verifying_key(vk)), verifier.rs:13-20) for the golden circuits' keys, and cg_pvk_load's
parser, which must refuse every byte string that is not exactly one PreparedVerifyingKey with CG_ERR_PARSE before any
HIP call - so these run without a GPU.  Pure CPU."""
import ctypes
import inspect
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import ark_files
import bn254_oracle as o
from conftest import ROOT
import verify_vectors as V

CG_ERR_PARSE, CG_ERR_INVALID_ARGUMENT = -7, -1


@pytest.fixture(scope="module")
def keys():
    out = {}
    for name in ("tiny", "d8", "dummy1024"):
        pk, _, _, _ = V.golden_vk(name)
        vk = pk["vk"]
        out[name] = (V.vk_bytes(vk), V.oracle_pvk_bytes(vk))
    return out


@pytest.mark.parametrize("name", ["tiny", "d8", "dummy1024"])
def test_prepare_verifying_key_matches_oracle(cc, keys, name):
    vkb, want = keys[name]
    got = cc.Groth16.prepare_verifying_key(vkb)
    assert len(got) == len(want)
    assert got == want


def test_prepare_verifying_key_identity_points(cc):
    """alpha = O gives alpha_g1_beta_g2 = 1; gamma = O a G2Prepared marked infinity (no coefficients)"""
    vk = V.synthetic_vk(3, 5, 7, 11, [13, 17])
    vk["alpha_g1"] = None
    vk["gamma_g2"] = None
    assert cc.Groth16.prepare_verifying_key(V.vk_bytes(vk)) == V.oracle_pvk_bytes(vk)


def test_prepare_verifying_key_rejects(cc):
    L = cc.lib()
    vkb = V.vk_bytes(V.synthetic_vk(3, 5, 7, 11, [13, 17]))
    n = ctypes.c_uint64()
    for bad in (vkb[:-1], vkb + b"\0", vkb[:100]):
        buf = (ctypes.c_uint8 * len(bad)).from_buffer_copy(bad)
        assert L.cg_prepare_verifying_key(buf, len(bad), None, 0, ctypes.byref(n)) == CG_ERR_PARSE
    buf = (ctypes.c_uint8 * len(vkb)).from_buffer_copy(vkb)
    assert L.cg_prepare_verifying_key(buf, len(vkb), None, 0, ctypes.byref(n)) == 0
    small = (ctypes.c_uint8 * 16)()
    assert L.cg_prepare_verifying_key(buf, len(vkb), small, 16, ctypes.byref(n)) == CG_ERR_INVALID_ARGUMENT


def _load_rc(cc, b):
    """cg_pvk_load's status; a handle that loaded (GPU present) is freed"""
    L = cc.lib()
    arr = (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) or b"\0")
    h = ctypes.c_void_p()
    rc = L.cg_pvk_load(ctypes.byref(h), arr, len(b), -1)
    if rc == 0:
        L.cg_pvk_free(h)
    return rc


def _layout(pvk: bytes):
    """offsets of the pieces of a serialized PreparedVerifyingKey"""
    r = ark_files._Rd(pvk)
    r.vk()
    vk_end = r.o
    ab_end = vk_end + 384
    gamma_at = ab_end
    n = struct.unpack_from("<Q", pvk, gamma_at)[0]
    delta_at = gamma_at + 8 + 192 * n + 1
    return vk_end, gamma_at, delta_at


def test_pvk_load_rejects_malformed_bytes_before_the_gpu(cc, keys):
    _, pvk = keys["d8"]
    vk_end, gamma_at, delta_at = _layout(pvk)
    Q = o.Q
    cases = {
        "empty": b"",
        "truncated by one": pvk[:-1],
        "truncated inside the vk": pvk[:200],
        "truncated inside alpha_g1_beta_g2": pvk[:vk_end + 100],
        "one trailing byte": pvk + b"\0",
        "two keys": pvk + pvk,
    }
    b = bytearray(pvk); struct.pack_into("<Q", b, vk_end - 8 - 64 * 3, 2 ** 62); cases["hostile gamma_abc length"] = bytes(b)
    b = bytearray(pvk); struct.pack_into("<Q", b, gamma_at, 2 ** 63 + 91); cases["hostile ell_coeffs length"] = bytes(b)
    b = bytearray(pvk); struct.pack_into("<Q", b, gamma_at, 90); cases["90 coefficients"] = bytes(b)
    b = bytearray(pvk); b[delta_at - 1] = 2; cases["infinity bool = 2"] = bytes(b)
    b = bytearray(pvk); b[vk_end:vk_end + 32] = Q.to_bytes(32, "little"); cases["alpha_g1_beta_g2 coordinate = q"] = bytes(b)
    b = bytearray(pvk); b[gamma_at + 8:gamma_at + 40] = (Q + 1).to_bytes(32, "little"); cases["line coefficient > q"] = bytes(b)
    b = bytearray(pvk); b[63] |= 0xC0; cases["alpha_g1 with both flags"] = bytes(b)
    b = bytearray(pvk); b[0:32] = (2 ** 256 - 1).to_bytes(32, "little"); cases["alpha_g1.x all ones"] = bytes(b)
    for what, bad in cases.items():
        assert _load_rc(cc, bad) == CG_ERR_PARSE, what


def test_pvk_load_survives_mutated_input(cc, keys):
    """the mutations tests/test_abi.py applies to the key parsers: corrupted, truncated, extended - an error or a key, never a
    crash; a truncation or an extension is always CG_ERR_PARSE"""
    rng = random.Random(11)
    _, pvk = keys["tiny"]
    for _ in range(400):
        b = bytearray(pvk)
        for _ in range(rng.choice([1, 2, 4])):
            b[rng.randrange(len(b))] = rng.choice([0, 0xFF, rng.randrange(256)])
        cut = rng.random() < 0.3
        if cut:
            b = b[:rng.randrange(len(b))]
        ext = rng.random() < 0.05
        if ext:
            b += bytes(rng.randrange(256) for _ in range(1 + rng.randrange(40)))
        rc = _load_rc(cc, bytes(b))
        if cut or ext:
            assert rc == CG_ERR_PARSE


def test_python_surface_is_bound(cc):
    from crescent_credentials_amd import api
    for name in ("cg_pvk_load", "cg_pvk_num_inputs", "cg_verify_batch", "cg_pvk_free", "cg_prepare_verifying_key"):
        assert name in api._SIGNATURES
        assert hasattr(cc.lib(), name)
    assert (cc.CG_VERIFY_REJECT, cc.CG_VERIFY_ACCEPT, cc.CG_VERIFY_MALFORMED) == (0, 1, 2)
    for m in ("prepare_verifying_key", "verify_with_processed_vk", "verify_batch"):
        assert callable(getattr(cc.Groth16, m))
    assert "verify" in inspect.signature(cc.create_client_state).parameters
    assert issubclass(cc.ProofRejected, cc.CrescentGpuError)
    with pytest.raises(cc.CrescentGpuError) as e:
        cc.PreparedVerifyingKey(b"\0" * 10)
    assert e.value.code == CG_ERR_PARSE


def test_c_caller_knows_verify():
    exe = os.path.join(ROOT, "integration", "c", "crescent_prove")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "--verify" in r.stderr
