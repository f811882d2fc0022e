"""The device-link maker without a GPU: cg_device_link_prove_batch and cg_device_link_prove_last_kernel_ms are declared,
exported, bound and declared to Rust; the struct's fields agree across the header, api.py and sys.rs; a null handle is an
argument error that touches nothing; and the k_dlm_* kernels that hold a sponge or a SHA block declare no private segment."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

from conftest import ROOT

CG_ERR_INVALID_ARGUMENT = -1
FIELDS = ["com1", "comz", "m", "pi0_c", "pi0_s", "pi1_c", "pi1_s"]


def test_entries_are_declared_exported_and_bound(cc):
    from crescent_credentials_amd import api
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crescent_gpu.h")).read(), flags=re.S)
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "sys.rs")).read()
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "lib.rs")).read()
    L = ctypes.CDLL(cc.library_path())
    for name, n_args in (("cg_device_link_prove_batch", 14), ("cg_device_link_prove_last_kernel_ms", 2)):
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert hasattr(L, name), name
        assert len(api._SIGNATURES[name][1]) == n_args, name
        r = re.search(r"pub fn %s\s*\((.*?)\)" % name, sys_rs, flags=re.S)
        assert r and len([a for a in r.group(1).split(",") if a.strip()]) == n_args, name
    assert re.search(r"#define CG_DEVICE_LINK_N_RAND 9\b", code) and api.CG_DEVICE_LINK_N_RAND == 9
    assert re.search(r"pub const CG_DEVICE_LINK_N_RAND: usize = 9;", sys_rs)
    for f in ("device_link_prove_batch_packed", "device_link_prove_batch", "device_link_openings"):
        assert callable(getattr(cc.Groth16, f))
    assert callable(cc.PreparedVerifyingKey.device_link_prove_last_kernel_ms)
    assert re.search(r"pub fn device_link_prove_batch\s*\(", lib_rs) and "sys::cg_device_link_prove_batch(" in lib_rs


def test_struct_fields_agree_across_header_python_and_rust():
    from crescent_credentials_amd import api
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crescent_gpu.h")).read(), flags=re.S)
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "sys.rs")).read()
    fields = re.search(r"typedef struct cg_device_link_made \{(.*?)\} cg_device_link_made;", code, flags=re.S).group(1)
    assert re.match(r"\s*uint8_t\s", fields)                       # rows the call writes: no const
    assert re.findall(r"\*(\w+)", fields) == FIELDS == [f for f, _ in api._CgDeviceLinkMade._fields_]
    assert all(ctypes.sizeof(t) == 8 for _, t in api._CgDeviceLinkMade._fields_)
    rust = re.search(r"pub struct cg_device_link_made \{(.*?)\n\}", sys_rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): \*mut u8,", rust) == FIELDS


def test_null_handle_is_an_argument_error(cc):
    from crescent_credentials_amd import api
    L = cc.lib()
    buf = np.full(512, 0xA5, np.uint8)
    p = buf.ctypes.data
    made = api._CgDeviceLinkMade(*[p] * 7)
    io = np.array([2, 2], np.uint8)
    assert L.cg_device_link_prove_batch(None, io.ctypes.data, 2, 0, 1, p, p, p, p, 32, 1, ctypes.byref(made), p, p) == CG_ERR_INVALID_ARGUMENT
    assert b"null" in L.cg_last_error()
    assert L.cg_device_link_prove_last_kernel_ms(None, (ctypes.c_float * 6)()) == CG_ERR_INVALID_ARGUMENT
    assert (buf == 0xA5).all()


def test_openings_are_cut_by_the_rule_of_the_showing_call(cc):
    """m = inputs[pos], r = rand[2 + committed_index] (csrc/show_make.hpp: mk_link_opening), on arrays that say where each
    byte came from; cg_show_rand_count is host arithmetic"""
    io, pos0, pos1 = [2, 1, 2, 2, 0], 2, 3
    n, n_rand = 3, cc.show_rand_count(io)
    inputs = np.zeros((n, len(io), 32), np.uint8)
    rand = np.zeros((n, n_rand, 32), np.uint8)
    for p in range(n):
        for i in range(len(io)):
            inputs[p, i] = (1, p, i) + (0,) * 29
        for j in range(n_rand):
            rand[p, j] = (2, p, j) + (0,) * 29
    got = cc.Groth16.device_link_openings(io, pos0, pos1, inputs.reshape(-1), rand.reshape(-1))
    assert got.shape == (n, 4, 32)
    for p in range(n):
        assert [tuple(int(x) for x in got[p, j, :3]) for j in range(4)] == [(1, p, 2), (2, p, 2 + 1), (1, p, 3), (2, p, 2 + 2)]
    io2 = [2, 2, 1, 2]                                             # the keys first, pos0 behind pos1
    got = cc.Groth16.device_link_openings(io2, 1, 0, inputs[:, :4].reshape(-1), rand[:, :cc.show_rand_count(io2)].reshape(-1))
    assert [tuple(int(x) for x in got[1, j, :3]) for j in range(4)] == [(1, 1, 1), (2, 1, 3), (1, 1, 0), (2, 1, 2)]


def test_maker_kernels_declare_no_private_segment(cc, tmp_path):
    """The Merlin sponge, and in k_dlm_pi0 the SHA-256 block and one coordinate's digits in its place, are addressed by
    run-time positions and would go to scratch as per-lane arrays; they are LDS.  Kernel metadata of the shipped gfx950 code
    objects only: nothing runs."""
    readelf, objdump = "/opt/rocm/lib/llvm/bin/llvm-readelf", "/opt/rocm/lib/llvm/bin/llvm-objdump"
    assert os.path.exists(readelf) and os.path.exists(objdump)
    work = os.path.join(str(tmp_path), "lib.so")
    shutil.copy(cc.library_path(), work)
    subprocess.run([objdump, "--offloading", work], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    want_lds = {"k_dlm_check": 0, "k_dlm_pi0": 64 * 200, "k_dlm_pi1": 64 * 200}
    all_six = {"k_dlm_check", "k_dlm_terms", "k_dlm_sum", "k_dlm_pi0", "k_dlm_lhs1", "k_dlm_pi1"}
    seen, named = {}, set()
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
                named |= set(re.findall(r"\d(k_dlm_[a-z0-9]+)E", nm.group(1)))
                for kernel in want_lds:
                    if re.search(r"\d%s[A-Z]" % kernel, nm.group(1)):
                        seen[kernel] = (int(ps.group(1)), dyn.group(1) if dyn else "false", int(lds.group(1)))
    assert named == all_six, named
    assert sorted(seen) == sorted(want_lds), seen
    for kernel, (private, dynamic, lds) in seen.items():
        assert private == 0 and dynamic == "false", "%s: %d bytes of scratch per lane (dynamic stack: %s)" % (kernel, private, dynamic)
        assert lds == want_lds[kernel], (kernel, lds)
