"""The C ABI of the T-256 entries (csrc/t256commit.hip), without a GPU: the six entries are declared in
include/crescent_gpu.h with the signatures the issue states, exported by the library, bound in api.py and declared to Rust;
null arguments and shape errors are argument errors that touch nothing; cg_t256_gens_load refuses a non-canonical coordinate,
a point off the curve, the identity and a bad count on the host, before any HIP call, so that all of it is seen here; and, from
the shipped code object's metadata, no kernel of the file declares a private segment."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

from conftest import ROOT
import t256_vectors as V

CG_ERR_INVALID_ARGUMENT = -1

ENTRIES = (("cg_t256_gens_load", 4), ("cg_t256_gens_free", 1), ("cg_t256_gens_info", 3), ("cg_t256_commit_rows_batch", 6),
           ("cg_hyrax_commit_batch", 7), ("cg_t256_commit_last_kernel_ms", 3))
DECLS = ("int cg_t256_gens_load(const uint8_t* g_xy, uint64_t n_gens, const uint8_t* h_xy, cg_t256_gens** out);",
         "void cg_t256_gens_free(cg_t256_gens* g);",
         "int cg_t256_gens_info(const cg_t256_gens* g, uint64_t* n_gens, uint64_t* table_bytes);",
         "int cg_t256_commit_rows_batch(cg_t256_gens* g, const uint8_t* scalars, const uint8_t* blinds, uint64_t n_rows, uint8_t* out33, "
         "uint8_t* status);",
         "int cg_hyrax_commit_batch(cg_t256_gens* g, uint32_t num_vars, const uint8_t* vars, const uint8_t* blinds, uint64_t n, uint8_t* out33, "
         "uint8_t* status);",
         "int cg_t256_commit_last_kernel_ms(cg_t256_gens* g, float ms[2], uint32_t* lanes_per_row);")


def test_entries_are_declared_exported_and_bound(cc):
    from crescent_credentials_amd import api
    header = open(os.path.join(ROOT, "include", "crescent_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "sys.rs")).read()
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "lib.rs")).read()
    L = ctypes.CDLL(cc.library_path())
    for name, n_args in ENTRIES:
        m = re.search(r"\b(?:int|void)\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert hasattr(L, name), name
        assert len(api._SIGNATURES[name][1]) == n_args, name
        r = re.search(r"pub fn %s\s*\((.*?)\)" % name, sys_rs, flags=re.S)
        assert r and len([a for a in r.group(1).split(",") if a.strip()]) == n_args, name
        assert "sys::%s(" % name in lib_rs, name
    flat = re.sub(r"\s+", " ", code)
    for decl in DECLS:
        assert decl in flat, decl
    assert "t256commit.hip" in open(os.path.join(ROOT, "crescent-credentials_amd", "build.py")).read()
    for f in ("commit_rows_batch", "hyrax_commit_batch", "commit_last_kernel_ms", "table_bytes"):
        assert hasattr(cc.T256Gens, f)
    # every entry carries the note that its byte forms are unverified readings
    block = header[header.index("pi2's witness commitment"):header.index("int cg_t256_commit_last_kernel_ms(")]
    assert block.count("UNVERIFIED") >= 4                                      # the forms' table, the loader and the two calls


def test_null_arguments_and_shape_errors_touch_nothing(cc):
    L = cc.lib()
    buf = np.full(4096, 0xA5, np.uint8)
    p = buf.ctypes.data
    h = ctypes.c_void_p(0x5A5A)
    assert L.cg_t256_gens_load(None, 1, p, ctypes.byref(h)) == CG_ERR_INVALID_ARGUMENT and b"null" in L.cg_last_error()
    assert L.cg_t256_gens_load(p, 1, None, ctypes.byref(h)) == CG_ERR_INVALID_ARGUMENT
    assert L.cg_t256_gens_load(p, 1, p, None) == CG_ERR_INVALID_ARGUMENT
    assert L.cg_t256_gens_info(None, ctypes.byref(ctypes.c_uint64()), ctypes.byref(ctypes.c_uint64())) == CG_ERR_INVALID_ARGUMENT
    assert L.cg_t256_commit_rows_batch(None, p, p, 1, p, p) == CG_ERR_INVALID_ARGUMENT and b"null" in L.cg_last_error()
    assert L.cg_hyrax_commit_batch(None, 2, p, p, 1, p, p) == CG_ERR_INVALID_ARGUMENT and b"null" in L.cg_last_error()
    assert L.cg_t256_commit_last_kernel_ms(None, (ctypes.c_float * 2)(), ctypes.byref(ctypes.c_uint32())) == CG_ERR_INVALID_ARGUMENT
    L.cg_t256_gens_free(None)
    assert (buf == 0xA5).all()


def test_the_loader_refuses_bad_points_on_the_host(cc):
    """every refusal comes before any HIP call, so a machine without a GPU sees it; *out is null afterwards"""
    L = cc.lib()
    gens = V.make_gens(0xAB1, 3)
    g, hb = gens.g_xy, gens.h_xy
    bad_y = V.be(gens.points[1][0]) + V.be((gens.points[1][1] + 1) % V.PT)
    big_x = V.be(V.PT) + V.be(gens.points[1][1])
    swap = lambda j, new: g[:64 * j] + new + g[64 * j + 64:]
    cases = ((swap(1, bad_y), hb, 3, b"G[1] is not on the curve"), (swap(2, big_x), hb, 3, b"G[2] has a coordinate"),
             (swap(0, bytes(64)), hb, 3, b"G[0] is the identity"), (g, bad_y, 3, b"h is not on the curve"), (g, bytes(64), 3, b"h is the identity"),
             (g, V.be(5) + V.be((1 << 256) - 1), 3, b"h has a coordinate"), (g, hb, 0, b"n_gens = 0"), (g, hb, 2056, b"n_gens = 2056"),
             (g, hb, 1 << 60, b"n_gens"))
    for g_xy, h_xy, n, msg in cases:
        ga, ha = np.frombuffer(g_xy, np.uint8).copy(), np.frombuffer(h_xy, np.uint8).copy()
        h = ctypes.c_void_p(0x5A5A)
        assert L.cg_t256_gens_load(ga.ctypes.data, n, ha.ctypes.data, ctypes.byref(h)) == CG_ERR_INVALID_ARGUMENT, msg
        assert msg in L.cg_last_error(), (msg, L.cg_last_error())
        assert not h.value


def test_t256_kernels_declare_no_private_segment(cc, tmp_path):
    """The partial of a lane stays in registers, the butterfly goes through LDS and digits are read through pointers: no
    scratch.  Kernel metadata of the shipped gfx950 code objects only: nothing runs."""
    readelf, objdump = "/opt/rocm/lib/llvm/bin/llvm-readelf", "/opt/rocm/lib/llvm/bin/llvm-objdump"
    assert os.path.exists(readelf) and os.path.exists(objdump)
    work = os.path.join(str(tmp_path), "lib.so")
    shutil.copy(cc.library_path(), work)
    subprocess.run([objdump, "--offloading", work], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    src = open(os.path.join(ROOT, "crescent-credentials_amd", "csrc", "t256commit.hip")).read()
    want = set(re.findall(r"__global__[^;{]*?\bvoid (k_t256_[a-z0-9_]+)\(", src))
    assert want == {"k_t256_check", "k_t256_rows", "k_t256_finish"}
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
            spill = re.search(r"\.vgpr_spill_count:\s+(\d+)", blk)
            if nm and ps:
                for kernel in re.findall(r"\d(k_t256_[a-z0-9_]+?)E", nm.group(1)):
                    seen[kernel] = (int(ps.group(1)), dyn.group(1) if dyn else "false", int(lds.group(1)), int(spill.group(1)) if spill else 0)
    assert set(seen) == want, seen
    for kernel, (private, dynamic, lds, spill) in seen.items():
        assert private == 0 and dynamic == "false" and spill == 0, "%s: %d bytes of scratch per lane (dynamic stack: %s)" % (kernel, private, dynamic)
    assert seen["k_t256_rows"][2] == 24 * 64 * 4                                # a projective point per lane, word-major
    assert seen["k_t256_check"][2] == 0 and seen["k_t256_finish"][2] == 0
