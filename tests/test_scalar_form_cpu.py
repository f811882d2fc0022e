"""Scalars in arkworks' in-memory form, the host side (no GPU): cg_scalars_convert against Python integers - the Montgomery
form of x is x * 2**256 % r - its refusals, the argument check of cg_qap_load_form, and the flag's value in the three places
that spell it (the header, the ctypes mirror, the Rust bindings)."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
CANONICAL, MONTGOMERY = 0, 1
INVALID = -1
SIZES = [0, 1, 255, 256, 257, 5000]          # the host split cuts ranges of at least 256: one range, a tail, many ranges


def _mont(x):
    return x * 2**256 % R


def _pack(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).copy()


def _ints(buf):
    b = bytes(buf)
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _values(n):
    """0, 1, r-1 first (as far as n allows), random ones after"""
    rng = random.Random(1000 + n)
    return ([0, 1, R - 1] + [rng.randrange(R) for _ in range(max(0, n - 3))])[:n]


@pytest.mark.parametrize("n", SIZES)
def test_convert_both_directions_against_python_ints(cc, n):
    vals = _values(n)
    canon = _pack(vals)
    mont = cc.scalars_convert(canon, CANONICAL, MONTGOMERY)
    assert _ints(mont) == [_mont(v) for v in vals]
    assert _ints(canon) == vals                                              # the input is not written
    assert _ints(cc.scalars_convert(mont, MONTGOMERY, CANONICAL)) == vals    # round trip
    # equal forms: a copy
    assert _ints(cc.scalars_convert(canon, CANONICAL, CANONICAL)) == vals
    assert _ints(cc.scalars_convert(mont, MONTGOMERY, MONTGOMERY)) == [_mont(v) for v in vals]


@pytest.mark.parametrize("n", SIZES)
def test_convert_in_place(cc, n):
    vals = _values(n)
    buf = _pack(vals)
    assert cc.scalars_convert(buf, CANONICAL, MONTGOMERY, out=buf) is buf
    assert _ints(buf) == [_mont(v) for v in vals]
    cc.scalars_convert(buf, MONTGOMERY, CANONICAL, out=buf)
    assert _ints(buf) == vals


def test_montgomery_form_of_small_values(cc):
    """the constants a reader can check by hand: 0 -> 0, 1 -> 2^256 mod r, r-1 -> r - (2^256 mod r)"""
    one = 2**256 % R
    assert _ints(cc.scalars_convert(_pack([0, 1, R - 1]), CANONICAL, MONTGOMERY)) == [0, one, R - one]
    assert _ints(cc.scalars_convert(_pack([0, one, R - one]), MONTGOMERY, CANONICAL)) == [0, 1, R - 1]


@pytest.mark.parametrize("in_form", [CANONICAL, MONTGOMERY])
@pytest.mark.parametrize("bad_value", [R, 2**256 - 1], ids=["r", "2^256-1"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_element_not_below_r_is_refused_with_its_index(cc, in_form, bad_value, n):
    L = cc.lib()
    for at in sorted({0, n - 1}):
        vals = _values(n)
        vals[at] = bad_value
        src = _pack(vals)
        out = np.full(32 * n, 0xAB, np.uint8)
        rc = L.cg_scalars_convert(src.ctypes.data, in_form, out.ctypes.data, 1 - in_form, n)
        msg = L.cg_last_error().decode()
        assert rc == INVALID and re.search(r"\belement %d\b" % at, msg), (at, rc, msg)
        assert bytes(out) == b"\xab" * (32 * n), "out was written"
        # in place: the vector is left as it was
        keep = src.copy()
        assert L.cg_scalars_convert(src.ctypes.data, in_form, src.ctypes.data, 1 - in_form, n) == INVALID
        assert bytes(src) == bytes(keep)
        # and through the Python wrapper
        with pytest.raises(cc.CrescentGpuError) as e:
            cc.scalars_convert(src, in_form, 1 - in_form)
        assert e.value.code == INVALID and "element %d " % at in str(e.value)


def test_the_first_bad_element_is_the_one_named(cc):
    n = 5000
    vals = _values(n)
    for at in (4999, 3000, 1234, 300):           # several bad elements, in different ranges of the host split
        vals[at] = R
    src = _pack(vals)
    out = np.zeros(32 * n, np.uint8)
    assert cc.lib().cg_scalars_convert(src.ctypes.data, CANONICAL, out.ctypes.data, MONTGOMERY, n) == INVALID
    assert "element 300 " in cc.lib().cg_last_error().decode()
    assert not out.any()


def test_convert_argument_errors(cc):
    L = cc.lib()
    buf = _pack([1, 2])
    for in_form, out_form in ((2, 0), (0, 2), (7, 7)):
        assert L.cg_scalars_convert(buf.ctypes.data, in_form, buf.ctypes.data, out_form, 2) == INVALID
        assert b"form" in L.cg_last_error()
    assert L.cg_scalars_convert(None, 0, buf.ctypes.data, 1, 2) == INVALID and b"null" in L.cg_last_error()
    assert L.cg_scalars_convert(buf.ctypes.data, 0, None, 1, 2) == INVALID
    assert L.cg_scalars_convert(None, 0, None, 1, 0) == 0                    # nothing to do
    assert _ints(buf) == [1, 2]


def test_qap_load_form_refuses_an_unknown_form_before_any_hip_call(cc):
    """as the argument tests of test_abi.py: this machine has no GPU, so an answer that names the argument was given before
    the library touched HIP"""
    from crescent_credentials_amd import api
    L = cc.lib()
    abc = (api._CgCsr * 3)()
    h = ctypes.c_void_p()
    for form in (2, 3, 0xFFFFFFFF):
        assert L.cg_qap_load_form(ctypes.byref(h), abc, 3, 4, 7, -1, form) == INVALID
        assert b"scalar_form" in L.cg_last_error() and not h.value
    # a known form goes on to the checks cg_qap_load makes
    for form in (CANONICAL, MONTGOMERY):
        assert L.cg_qap_load_form(ctypes.byref(h), abc, 3, 4, 7, -1, form) == INVALID and b"null row_ptr" in L.cg_last_error()
        assert L.cg_qap_load_form(ctypes.byref(h), abc, 0, 4, 7, -1, form) == INVALID
    assert L.cg_qap_load_form(None, abc, 3, 4, 7, -1, 0) == INVALID


def test_circuit_load_knows_the_flag(cc):
    """512 is no longer an unknown bit: the load goes on to its next check (the key's pointers), alone and next to other flags"""
    from crescent_credentials_amd import api
    L = cc.lib()
    pk = api._CgProvingKey()
    pk.coord_form = 0
    pk.a_len = pk.b_g1_len = pk.b_g2_len = 7
    pk.l_len = 4
    pk.h_len = 7
    abc = (api._CgCsr * 3)()
    h = ctypes.c_void_p()
    for flags in (512, 512 | 1, 512 | 64 | 128, 512 | 8 | 4):
        opt = api._CgOptions(device=-1, flags=flags)
        rc = L.cg_circuit_load(ctypes.byref(h), ctypes.byref(pk), abc, 3, 4, 7, ctypes.byref(opt))
        assert rc == INVALID and b"null key point" in L.cg_last_error(), flags
    opt = api._CgOptions(device=-1, flags=512 | 1024)
    assert L.cg_circuit_load(ctypes.byref(h), ctypes.byref(pk), abc, 3, 4, 7, ctypes.byref(opt)) == INVALID
    assert b"unknown bits in flags" in L.cg_last_error()


def test_flag_value_in_header_python_and_rust(cc):
    from crescent_credentials_amd import api
    hdr = open(os.path.join(ROOT, "include", "crescent_gpu.h")).read()
    m = re.search(r"\bCG_FLAG_SCALARS_MONTGOMERY\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == 512
    assert api.CG_FLAG_SCALARS_MONTGOMERY == 512 == cc.CG_FLAG_SCALARS_MONTGOMERY
    rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "sys.rs")).read()
    assert re.search(r"pub const CG_FLAG_SCALARS_MONTGOMERY: i32 = 512;", rs)
    assert re.search(r"pub fn cg_qap_load_form\s*\(", rs) and re.search(r"pub fn cg_scalars_convert\s*\(", rs)
    # the shim loads with the flag, hands over Fr.0 limb by limb, and pins the element size the library reads
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "lib.rs")).read()
    assert "sys::CG_FLAG_SCALARS_MONTGOMERY" in lib_rs and "sys::cg_qap_load_form" in lib_rs and "Fr::new_unchecked(BigInt(" in lib_rs
    assert re.search(r"const _: \(\) = assert!\(std::mem::size_of::<Fr>\(\) == 32\);", lib_rs)
    body = re.search(r"pub fn create_proof\(.*?\n    }\n", lib_rs, flags=re.S).group(0)
    code = re.sub(r"//[^\n]*", "", body.split("let (rb, sb)")[0])
    assert "into_bigint" not in code and "put_fr(" in code, "create_proof still converts the assignment on the host"
