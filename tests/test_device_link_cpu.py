"""The device link without a GPU: the new entries are declared, exported, bound and declared to Rust; the host-only
cg_revealed_digest_batch (creds/src/lib.rs:590-603) against hashlib and a Python `bits_to_num` (utils.rs:78-94); and the
argument errors of both entries that need no device."""
import ctypes
import hashlib
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT

CG_ERR_INVALID_ARGUMENT = -1
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def bits_to_num(b: bytes) -> int:
    """utils.rs:78-94: the bits of the bytes, most significant bit of each byte first; bit i of the string has weight 2^i;
    248 bits are read"""
    bits = [(byte >> i) & 1 for byte in b for i in range(7, -1, -1)]
    return sum(bit << i for i, bit in enumerate(bits[:248]))


def want_row(item: bytes) -> bytes:
    v = bits_to_num(hashlib.sha256(item).digest()[:31])
    assert v < R
    return v.to_bytes(32, "little")


def test_entries_are_declared_exported_and_bound(cc):
    from crescent_credentials_amd import api
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crescent_gpu.h")).read(), flags=re.S)
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "sys.rs")).read()
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "lib.rs")).read()
    L = ctypes.CDLL(cc.library_path())
    for name, n_args in (("cg_device_link_verify_batch", 12), ("cg_device_link_last_kernel_ms", 2), ("cg_revealed_digest_batch", 4)):
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert hasattr(L, name), name
        assert len(api._SIGNATURES[name][1]) == n_args, name
        assert re.search(r"pub fn %s\s*\(" % name, sys_rs), name
    fields = re.search(r"typedef struct cg_device_link_rows \{(.*?)\} cg_device_link_rows;", code, flags=re.S).group(1)
    names = re.findall(r"\*(\w+)", fields)
    assert names == ["com1", "comz", "h_q", "m", "pi0_c", "pi0_s", "pi1_c", "pi1_s"] == [f for f, _ in api._CgDeviceLinkRows._fields_]
    rust = re.search(r"pub struct cg_device_link_rows \{(.*?)\n\}", sys_rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): \*const u8,", rust) == names
    for f in ("device_link_verify_batch_packed", "device_link_verify_batch", "revealed_digest_batch"):
        assert callable(getattr(cc.Groth16, f))
    assert re.search(r"pub fn device_link_verify_batch\s*\(", lib_rs) and re.search(r"pub fn revealed_digest_batch\s*\(", lib_rs)


@pytest.mark.parametrize("length", [0, 1, 55, 56, 63, 64, 65, 119, 120, 1000])
def test_revealed_digest_of_one_item(cc, length):
    item = bytes(random.Random(0x4E7 + length).randrange(256) for _ in range(length))
    out = cc.Groth16.revealed_digest_batch([item])
    assert out.shape == (1, 32) and out.tobytes() == want_row(item)
    assert out[0, 31] == 0


def test_revealed_digest_mirrors_the_bits_of_each_byte(cc):
    d = hashlib.sha256(b"abc").digest()
    out = cc.Groth16.revealed_digest_batch([b"abc"]).tobytes()
    assert out == bytes(int("{:08b}".format(b)[::-1], 2) for b in d[:31]) + b"\0"


def test_revealed_digest_of_ten_items_with_an_empty_one_between(cc):
    rng = random.Random(0x10E)
    items = [bytes(rng.randrange(256) for _ in range(n)) for n in (3, 64, 0, 17, 55, 56, 200, 1, 119, 1000)]
    assert len(items) == 10 and items[1] and not items[2] and items[3]
    out = cc.Groth16.revealed_digest_batch(items)
    assert out.tobytes() == b"".join(want_row(b) for b in items)
    assert cc.Groth16.revealed_digest_batch([]).shape == (0, 32)


def test_revealed_digest_argument_errors_touch_nothing(cc):
    L = cc.lib()
    data = np.frombuffer(b"0123456789", np.uint8).copy()
    out = np.full(64, 0xA5, np.uint8)
    off = lambda *v: np.array(v, np.uint64).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    assert L.cg_revealed_digest_batch(data.ctypes.data, off(0, 4, 10), 2, None) == CG_ERR_INVALID_ARGUMENT
    assert L.cg_revealed_digest_batch(data.ctypes.data, None, 2, out.ctypes.data) == CG_ERR_INVALID_ARGUMENT
    assert L.cg_revealed_digest_batch(data.ctypes.data, off(0, 6, 4), 2, out.ctypes.data) == CG_ERR_INVALID_ARGUMENT
    assert b"offsets" in L.cg_last_error()
    assert L.cg_revealed_digest_batch(None, off(0, 4, 10), 2, out.ctypes.data) == CG_ERR_INVALID_ARGUMENT
    assert (out == 0xA5).all()
    assert L.cg_revealed_digest_batch(None, off(0, 0, 0), 2, out.ctypes.data) == 0          # two empty items need no data
    assert out.tobytes() == want_row(b"") * 2
    assert L.cg_revealed_digest_batch(None, None, 0, None) == 0


def test_device_link_kernels_declare_no_private_segment(cc, tmp_path):
    """The SHA-256 block, one coordinate's digits and the Merlin sponge are addressed by run-time positions and would go to
    scratch as per-lane arrays; they are LDS.  Kernel metadata of the shipped gfx950 code objects only: nothing runs."""
    import shutil
    import subprocess
    readelf, objdump = "/opt/rocm/lib/llvm/bin/llvm-readelf", "/opt/rocm/lib/llvm/bin/llvm-objdump"
    assert os.path.exists(readelf) and os.path.exists(objdump)
    work = os.path.join(str(tmp_path), "lib.so")
    shutil.copy(cc.library_path(), work)
    subprocess.run([objdump, "--offloading", work], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    want_lds = {"k_dl_check": 64 * (64 + 84), "k_dl_terms": 0, "k_dl_sum": 0, "k_dl_challenge": 64 * 200}
    seen = {}
    for f in sorted(os.listdir(str(tmp_path))):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([readelf, "--notes", os.path.join(str(tmp_path), f)], capture_output=True, text=True, check=True).stdout
        for blk in re.split(r"\n\s*- \.", notes):
            nm = re.search(r"\.name:\s+(\S+)", blk)
            ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            dyn = re.search(r"\.uses_dynamic_stack:\s+(\w+)", blk)
            lds = re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk)
            if nm and ps:
                for kernel in want_lds:
                    if re.search(r"\d%s[A-Z]" % kernel, nm.group(1)):
                        seen[kernel] = (int(ps.group(1)), dyn.group(1) if dyn else "false", int(lds.group(1)))
    assert sorted(seen) == sorted(want_lds), seen
    for kernel, (private, dynamic, lds) in seen.items():
        assert private == 0 and dynamic == "false", "%s: %d bytes of scratch per lane (dynamic stack: %s)" % (kernel, private, dynamic)
        assert lds == want_lds[kernel], (kernel, lds)


def test_device_link_null_handle_is_an_argument_error(cc):
    from crescent_credentials_amd import api
    L = cc.lib()
    buf = np.full(256, 0xA5, np.uint8)
    p = buf.ctypes.data
    rows = api._CgDeviceLinkRows(*[p] * 8)
    io = np.array([2, 2], np.uint8)
    assert L.cg_device_link_verify_batch(None, io.ctypes.data, 2, 0, 1, p, ctypes.byref(rows), 32, 1, p, p, p) == CG_ERR_INVALID_ARGUMENT
    assert L.cg_device_link_last_kernel_ms(None, (ctypes.c_float * 4)()) == CG_ERR_INVALID_ARGUMENT
    assert (buf == 0xA5).all()
