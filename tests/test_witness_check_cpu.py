"""CPU-side checks of the witness check's interface (cg_check_witness, cg_qap_check_witness, CG_FLAG_CHECK_WITNESS):
the header declares it, the library exports it, the ctypes and Rust mirrors of cg_witness_report have the header's
layout, the entry points refuse a null handle before any HIP call, and the C caller knows --check-witness.  No GPU."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "crescent_gpu.h")
FIELDS = ("n_unsatisfied", "first_unsatisfied", "a", "b", "c", "check_ms", "reserved")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def test_header_declares_the_report_the_two_functions_and_the_flag():
    h = _header()
    body = re.search(r"typedef struct cg_witness_report \{(.*?)\} cg_witness_report;", h, flags=re.S).group(1)
    decls = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert decls == ["uint64_t n_unsatisfied", "uint64_t first_unsatisfied", "uint8_t a[32]", "uint8_t b[32]", "uint8_t c[32]",
                     "float check_ms", "int32_t reserved[7]"]
    assert re.search(r"int cg_check_witness\(cg_ctx\* ctx, const void\* full_assignment, int assignment_on_device, cg_witness_report\* report\);", h)
    assert re.search(r"int cg_qap_check_witness\(cg_qap_ctx\* ctx, const void\* full_assignment, int assignment_on_device, cg_witness_report\* report\);", h)
    assert re.search(r"CG_FLAG_CHECK_WITNESS = 256\b", h)
    assert re.search(r"CG_ERR_UNSATISFIED = -8\b", h)
    # the status code is no longer a debug-only promise
    assert "(debug check only)" not in open(HDR).read()


def test_library_exports_the_entry_points_and_refuses_null_without_hip(cc):
    L = cc.lib()
    for name in ("cg_check_witness", "cg_qap_check_witness"):
        assert hasattr(L, name), name
        w = (ctypes.c_uint8 * 32)()
        assert getattr(L, name)(None, w, 0, None) == -1              # CG_ERR_INVALID_ARGUMENT, before any HIP call
        assert b"null" in L.cg_last_error()
    assert cc.CG_FLAG_CHECK_WITNESS == 256 and cc.CG_ERR_UNSATISFIED == -8
    assert issubclass(cc.UnsatisfiedWitness, cc.CrescentGpuError)
    e = cc.UnsatisfiedWitness("constraint 3 of 8 is not satisfied (1 in all)")
    assert e.code == -8 and e.report is None
    rep = cc.WitnessReport(0, None, None, None, None, 0.0)
    assert rep.satisfied and not cc.WitnessReport(2, 5, 1, 2, 3, 0.1).satisfied
    for cls, names in ((cc.Prover, ("check_witness",)), (cc.QapContext, ("check_witness",)),
                       (cc.CircomCircuit, ("is_satisfied", "which_is_unsatisfied"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)


def test_ctypes_mirror_has_the_headers_size_and_offsets(tmp_path):
    from crescent_credentials_amd import api
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <crescent_gpu.h>\nint main(void) {\n'
                   '  printf("%zu", sizeof(cg_witness_report));\n' +
                   "".join('  printf(" %%zu", offsetof(cg_witness_report, %s));\n' % f for f in FIELDS) +
                   '  printf("\\n");\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    nums = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    R = api._CgWitnessReport
    assert [f for f, _ in R._fields_] == list(FIELDS)
    assert nums[0] == ctypes.sizeof(R) == 144
    assert nums[1:] == [getattr(R, f).offset for f in FIELDS]
    assert ("cg_check_witness" in api._SIGNATURES) and ("cg_qap_check_witness" in api._SIGNATURES)


def test_rust_shim_carries_the_struct_the_functions_and_the_flag():
    rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "sys.rs")).read()
    body = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^\]]*\)\]\s*)?pub struct cg_witness_report \{(.*?)\n\}", rs, flags=re.S).group(1)
    rust = [(f, " ".join(t.split())) for f, t in re.findall(r"pub (\w+):\s*([^,\n]+),", body)]
    assert rust == [("n_unsatisfied", "u64"), ("first_unsatisfied", "u64"), ("a", "[u8; 32]"), ("b", "[u8; 32]"), ("c", "[u8; 32]"),
                    ("check_ms", "f32"), ("reserved", "[i32; 7]")]
    for fn, handle in (("cg_check_witness", "cg_ctx"), ("cg_qap_check_witness", "cg_qap_ctx")):
        m = re.search(r"pub fn %s\s*\((.*?)\)\s*->\s*c_int;" % fn, rs, flags=re.S)
        assert m, fn
        args = [" ".join(a.split(":", 1)[1].split()) for a in m.group(1).split(",") if a.strip()]
        assert args == ["*mut %s" % handle, "*const c_void", "c_int", "*mut cg_witness_report"], (fn, args)
    assert re.search(r"pub const CG_FLAG_CHECK_WITNESS: i32 = 256;", rs)
    assert re.search(r"pub const CG_ERR_UNSATISFIED: c_int = -8;", rs)
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "lib.rs")).read()
    assert re.search(r"pub fn check_witness\(&self, full_assignment: &\[Fr\]\)", lib_rs) and "sys::cg_check_witness" in lib_rs


def test_c_caller_knows_the_option():
    src = open(os.path.join(ROOT, "integration", "c", "crescent_prove.c")).read()
    usage = re.search(r'"usage:.*?argv\[0\]\);', src, flags=re.S).group(0)
    assert "[--check-witness]" in usage
    assert '"--check-witness"' in src and "CG_FLAG_CHECK_WITNESS" in src and "cg_check_witness(" in src
    exe = os.path.join(ROOT, "integration", "c", "crescent_prove")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "--check-witness" in r.stderr


def test_flagged_load_without_matrices_is_refused_by_the_flags_name(cc):
    """a load that asks for the check and hands over no matrices is told so before anything else of the key is looked at"""
    from crescent_credentials_amd import api
    L = cc.lib()
    pk = api._CgProvingKey()
    pk.a_len = pk.b_g1_len = pk.b_g2_len = 7
    pk.l_len, pk.h_len = 4, 7
    abc = (api._CgCsr * 3)()
    h = ctypes.c_void_p()
    opt = api._CgOptions(device=-1, flags=cc.CG_FLAG_CHECK_WITNESS)
    assert L.cg_circuit_load(ctypes.byref(h), ctypes.byref(pk), abc, 3, 4, 7, ctypes.byref(opt)) == -1
    msg = L.cg_last_error()
    assert b"CG_FLAG_CHECK_WITNESS" in msg and b"matrix 0" in msg and not msg.startswith(b"CG_")
    opt = api._CgOptions(device=-1, flags=cc.CG_FLAG_CHECK_WITNESS | 32, shard_count=2)
    assert L.cg_circuit_load(ctypes.byref(h), ctypes.byref(pk), abc, 3, 4, 7, ctypes.byref(opt)) == -1
    assert b"CG_FLAG_H_SCALARS_EXTERNAL" in L.cg_last_error()
