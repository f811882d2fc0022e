"""The C ABI of the P-256 entries (csrc/p256tu.hip), without a GPU: cg_p256_tu_batch, cg_p256_rtu_batch and
cg_p256_last_kernel_ms are declared in include/crescent_gpu.h with the signatures the issue states, exported by the library,
bound in api.py and declared to Rust; the new status CG_P256_BAD_SIGNATURE is 3 beside CG_SHOW_MADE = 1 and
CG_SHOW_MALFORMED = 2, which keep their values; a null argument is an argument error that touches nothing."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

CG_ERR_INVALID_ARGUMENT = -1

ENTRIES = (("cg_p256_tu_batch", 7), ("cg_p256_rtu_batch", 9), ("cg_p256_last_kernel_ms", 3))


def test_entries_are_declared_exported_and_bound(cc):
    from crescent_credentials_amd import api
    header = open(os.path.join(ROOT, "include", "crescent_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "sys.rs")).read()
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "lib.rs")).read()
    L = ctypes.CDLL(cc.library_path())
    for name, n_args in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert hasattr(L, name), name
        assert len(api._SIGNATURES[name][1]) == n_args, name
        r = re.search(r"pub fn %s\s*\((.*?)\)" % name, sys_rs, flags=re.S)
        assert r and len([a for a in r.group(1).split(",") if a.strip()]) == n_args, name
        assert "sys::%s(" % name in lib_rs, name
    # the signatures as declared, token for token
    flat = re.sub(r"\s+", " ", code)
    for decl in ("int cg_p256_tu_batch(cg_pvk* k, const uint8_t* r_xy, const uint8_t* digest, uint64_t n, uint8_t* t_xy, uint8_t* u_xy, uint8_t* status);",
                 "int cg_p256_rtu_batch(cg_pvk* k, const uint8_t* q_xy, const uint8_t* sig, const uint8_t* digest, uint64_t n, uint8_t* r_xy, uint8_t* t_xy, "
                 "uint8_t* u_xy, uint8_t* status);",
                 "int cg_p256_last_kernel_ms(cg_pvk* k, float ms[3], uint32_t* uploads);"):
        assert decl in flat, decl
    for f in ("p256_tu_batch", "p256_rtu_batch", "p256_tu", "p256_rtu"):
        assert callable(getattr(cc.Groth16, f))
    assert callable(cc.PreparedVerifyingKey.p256_last_kernel_ms)
    # the new status beside the two it joins, whose values stay
    for name, value in (("CG_SHOW_MADE", 1), ("CG_SHOW_MALFORMED", 2), ("CG_P256_BAD_SIGNATURE", 3)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), code), name
        assert getattr(api, name) == value
    assert "pub const CG_P256_BAD_SIGNATURE: u8 = 3;" in sys_rs


def test_null_arguments_are_argument_errors(cc):
    L = cc.lib()
    buf = np.full(512, 0xA5, np.uint8)
    p = buf.ctypes.data
    assert L.cg_p256_tu_batch(None, p, p, 1, p, p, p) == CG_ERR_INVALID_ARGUMENT and b"null" in L.cg_last_error()
    assert L.cg_p256_rtu_batch(None, p, p, p, 1, p, p, p, p) == CG_ERR_INVALID_ARGUMENT and b"null" in L.cg_last_error()
    assert L.cg_p256_last_kernel_ms(None, (ctypes.c_float * 3)(), ctypes.byref(ctypes.c_uint32())) == CG_ERR_INVALID_ARGUMENT
    assert (buf == 0xA5).all()
