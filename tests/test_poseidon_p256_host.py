"""csrc/fp256.hpp and csrc/poseidon_p256.hpp on the HOST (g++ build of tests/cpp/test_poseidon_p256.cpp): the field operations
against Python integers at the prime's edges - (p - 1) + (p - 1) and (p - 1)^2 among them, where the sum and the Montgomery
accumulator pass 2^256 and field.hpp's Fp<P> would drop a word -, the 199 elements a handle uploads, the permutation and h_Q
against tests/poseidon_vectors.py, and the inputs of tests/steer_vectors.py, each of which takes one add or product site of the
permutation's first round, or of h_Q's entry, into the rare branch of f256_reduce_once.  The same program, built with the address and undefined-behaviour sanitizers, answers the
same requests on its own.  Then, without running anything: the new entries are declared, exported, bound and declared to
Rust, a null handle is an argument error, and the three h_Q kernels declare no private segment.  Pure CPU."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import poseidon_vectors as PV
import steer_vectors as S

P, R = PV.P256, PV.BN254_FR
SRC = os.path.join(ROOT, "tests", "cpp", "test_poseidon_p256.cpp")
EDGES = [0, 1, 2, P - 1, P - 2, 1 << 255, (1 << 255) + 1, (1 << 255) - 1, 1 << 224, 1 << 192, (1 << 96) - 1]
CG_ERR_INVALID_ARGUMENT = -1


def fe(v):
    return int(v).to_bytes(32, "little").hex()


def ask_all(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = r.stdout.split()
    assert len(out) == len(lines) and "ERR" not in out, r.stdout[-2000:]
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("poseidon_p256") / "test_poseidon_p256")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", path, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


# ---- the field ---------------------------------------------------------------------------------------------------------------
def field_lines(n_random):
    rng = random.Random(0xF256)
    pairs = [(a, b) for a in EDGES for b in EDGES] + [(rng.randrange(P), rng.randrange(P)) for _ in range(n_random)]
    assert (P - 1, P - 1) in pairs
    lines, want = [], []
    for a, b in pairs:
        lines += ["add %s %s" % (fe(a), fe(b)), "sub %s %s" % (fe(a), fe(b)), "mul %s %s" % (fe(a), fe(b))]
        want += [fe((a + b) % P), fe((a - b) % P), fe(a * b % P)]
    for a in EDGES + [rng.randrange(P) for _ in range(n_random // 10)]:
        lines += ["sqr %s" % fe(a), "pow5 %s" % fe(a)]
        want += [fe(a * a % P), fe(pow(a, 5, P))]
    for v, ok in ((0, 1), (P - 1, 1), (P, 0), (P + 1, 0), ((1 << 256) - 1, 0), (1 << 255, 1), (P - (1 << 96), 1), (P + (1 << 128), 0)):
        lines.append("below %s" % fe(v))
        want.append(str(ok))
    lines.append("r2")
    want.append("1")
    return lines, want


def test_field_operations_at_the_edges_and_on_random_pairs(exe):
    lines, want = field_lines(10000)
    got = ask_all(exe, lines)
    for line, g, w in zip(lines, got, want):
        assert g == w, line
    assert 2 * (P - 1) >= 1 << 256                                             # the sum Fp<P> cannot hold


# ---- the constants, the permutation, h_Q ---------------------------------------------------------------------------------------
def test_all_199_uploaded_elements_equal_pythons(exe):
    got = ask_all(exe, ["consts"])[0]
    want = PV.table()
    assert len(want) == 189 + 9 + 1 and len(got) == 64 * len(want)
    for i, w in enumerate(want):
        assert got[64 * i:64 * i + 64] == fe(w), i


def poseidon_lines(n_random):
    rng = random.Random(0x9053)
    c = PV.p256()
    lines, want = [], []
    states = [[0, 0, 0], [P - 1, P - 1, P - 1]] + [[rng.randrange(P) for _ in range(3)] for _ in range(n_random)]
    for st in states:
        lines.append("permute " + "".join(fe(x) for x in st))
        want.append("".join(fe(x) for x in PV.permute(c, st)))
    for bad in ([P, 0, 0], [0, (1 << 256) - 1, 0], [1, 2, P]):
        lines.append("permute " + "".join(fe(x) for x in bad))
        want.append("malformed")
    triples = [(0, 0, 0), (R - 1, R - 1, R - 1), (1, 2, 3)] + [tuple(rng.randrange(R) for _ in range(3)) for _ in range(n_random)]
    for q in triples:
        lines.append("hq " + "".join(fe(x) for x in q))
        want.append(PV.hq(*q).hex())
    for bad in ((R, 0, 0), (0, R, 0), (0, 0, R), (P - 1, 1, 1)):
        lines.append("hq " + "".join(fe(x) for x in bad))
        want.append("malformed")
    return lines, want


def test_permutation_and_hq_on_256_random_inputs(exe):
    lines, want = poseidon_lines(256)
    got = ask_all(exe, lines)
    for line, g, w in zip(lines, got, want):
        assert g == w, line[:80]
    assert "hq " + fe(1) + fe(2) + fe(3) in lines
    assert want[lines.index("hq " + fe(1) + fe(2) + fe(3))] == "b4c83f5ebbc2a8a6c913d1361168ceee2d3796453258470cb7ac7c3abeb24ab5"


# ---- inputs steered to the rare branch (tests/steer_vectors.py; tests/test_steer_vectors_cpu.py shows that each hits its site) --------
def steered_lines(every=1):
    """whole rows: `permute` on every steered state and `hq` on every steered triple"""
    c = PV.p256()
    lines, want = [], []
    for name, _ in S.POSEIDON_FAMILIES:
        for v in S.poseidon_families()[name][::every]:
            lines.append("permute " + "".join(fe(x) for x in v.state))
            want.append("".join(fe(x) for x in PV.permute(c, list(v.state))))
    for v in S.hq_vectors()[::every]:
        lines.append("hq " + "".join(fe(x) for x in v.q))
        want.append(PV.hq(*v.q).hex())
    return lines, want


def site_lines(every=1):
    """the steered site alone, as one `add`, `sqr` or `mul` on the values it meets"""
    c = PV.p256()
    lines, want = [], []
    vecs = [v for name, _ in S.POSEIDON_FAMILIES for v in S.poseidon_families()[name]]
    for v in vecs[::every]:
        a = [(x + k) % P for x, k in zip(v.state, c.rc[:3])]
        s = [pow(x, 5, P) for x in a]
        kind, i = v.site[0], v.site[1]
        if kind == "add_rc":
            ops = [("add", v.state[i], c.rc[i])]
        elif kind == "sqr":
            ops = [("sqr", a[i]), ("pow5", a[i])]
        elif kind == "sqr_sqr":
            ops = [("sqr", a[i] * a[i] % P), ("pow5", a[i])]
        elif kind == "mul_a4_a":
            ops = [("mul", pow(a[i], 4, P), a[i]), ("pow5", a[i])]
        elif kind == "mds_mul":
            ops = [("mul", c.mds[i // 3][i % 3], s[i % 3])]
        else:
            t = [c.mds[i][j] * s[j] % P for j in range(3)]
            ops = [("add", t[0], t[1])] if v.site[2] == 0 else [("add", (t[0] + t[1]) % P, t[2])]
        for op in ops:
            x = op[1:]
            lines.append(op[0] + " " + " ".join(fe(y) for y in x))
            want.append(fe({"add": lambda: x[0] + x[1], "mul": lambda: x[0] * x[1], "sqr": lambda: x[0] * x[0], "pow5": lambda: pow(x[0], 5, P)}[op[0]]() % P))
    # P-256's coordinates at the entry of p256_read_point and p256_on_curve: from_words (inside `sqr`), x + x and 2x + x
    for v in S.p256_families()["entry_points"][::every]:
        f = S.facts(v)
        if "point" in f and v.kind == "tu":
            x, y = f["point"]
            lines += ["sqr " + fe(x), "sqr " + fe(y), "add %s %s" % (fe(x), fe(x)), "add %s %s" % (fe(2 * x % P), fe(x))]
            want += [fe(x * x % P), fe(y * y % P), fe(2 * x % P), fe(3 * x % P)]
    return lines, want


def test_steered_states_and_triples_byte_for_byte(exe):
    lines, want = steered_lines()
    assert len(lines) == sum(S.POSEIDON_COUNTS.values()) == 33
    got = ask_all(exe, lines)
    for line, g, w in zip(lines, got, want):
        assert g == w, line[:80]


def test_steered_sites_one_operation_each(exe):
    lines, want = site_lines()
    assert len(lines) == 9 + 9 * 2 + 3 + 6 + 10 * 4
    got = ask_all(exe, lines)
    for line, g, w in zip(lines, got, want):
        assert g == w, line


def test_sanitized_build_answers_the_same(tmp_path):
    path = str(tmp_path / "test_poseidon_p256_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", path, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines, want = field_lines(500)
    for a, b in (poseidon_lines(16), steered_lines(3), site_lines(3)):
        lines, want = lines + a, want + b
    lines, want = lines + ["consts"], want + ["".join(fe(x) for x in PV.table())]
    assert ask_all(path, lines) == want


# ---- the entries, without a GPU --------------------------------------------------------------------------------------------------
ENTRIES = (("cg_poseidon_p256_permute_batch", 5), ("cg_hq_batch", 5), ("cg_device_link_prove_hq_batch", 13), ("cg_hq_last_kernel_ms", 3))


def test_entries_are_declared_exported_and_bound(cc):
    from crescent_credentials_amd import api
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crescent_gpu.h")).read(), flags=re.S)
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
    for f in ("poseidon_p256_permute_batch_packed", "hq_batch_packed", "device_link_prove_hq_batch_packed", "device_link_prove_hq_batch"):
        assert callable(getattr(cc.Groth16, f))
    assert callable(cc.PreparedVerifyingKey.hq_last_kernel_ms)
    # the proving entry as it was: fourteen arguments, h_q and h_len among them
    m = re.search(r"\bint\s+cg_device_link_prove_batch\s*\((.*?)\)\s*;", code, flags=re.S)
    assert len(m.group(1).split(",")) == 14 and "h_len" in m.group(1)


def test_null_handle_is_an_argument_error(cc):
    from crescent_credentials_amd import api
    L = cc.lib()
    buf = np.full(512, 0xA5, np.uint8)
    p = buf.ctypes.data
    made = api._CgDeviceLinkMade(*[p] * 7)
    io = np.array([2, 2], np.uint8)
    assert L.cg_poseidon_p256_permute_batch(None, p, 1, p, p) == CG_ERR_INVALID_ARGUMENT and b"null" in L.cg_last_error()
    assert L.cg_hq_batch(None, p, 1, p, p) == CG_ERR_INVALID_ARGUMENT and b"null" in L.cg_last_error()
    assert L.cg_device_link_prove_hq_batch(None, io.ctypes.data, 2, 0, 1, p, p, p, 1, ctypes.byref(made), p, p, p) == CG_ERR_INVALID_ARGUMENT
    assert b"null" in L.cg_last_error()
    assert L.cg_hq_last_kernel_ms(None, (ctypes.c_float * 2)(), ctypes.byref(ctypes.c_uint32())) == CG_ERR_INVALID_ARGUMENT
    assert (buf == 0xA5).all()


def test_hq_kernels_declare_no_private_segment(cc, tmp_path):
    """The Poseidon state is three elements in registers and the round constants are read at a wave-uniform address: no
    per-lane array, so no scratch.  Kernel metadata of the shipped gfx950 code objects only: nothing runs."""
    readelf, objdump = "/opt/rocm/lib/llvm/bin/llvm-readelf", "/opt/rocm/lib/llvm/bin/llvm-objdump"
    assert os.path.exists(readelf) and os.path.exists(objdump)
    work = os.path.join(str(tmp_path), "lib.so")
    shutil.copy(cc.library_path(), work)
    subprocess.run([objdump, "--offloading", work], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    want = {"k_hq_permute", "k_hq_hash", "k_hq_link"}
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
                for kernel in re.findall(r"\d(k_hq_[a-z0-9]+)E", nm.group(1)):
                    seen[kernel] = (int(ps.group(1)), dyn.group(1) if dyn else "false", int(lds.group(1)), int(spill.group(1)) if spill else 0)
    assert set(seen) == want, seen
    for kernel, (private, dynamic, lds, spill) in seen.items():
        assert private == 0 and dynamic == "false" and spill == 0, "%s: %d bytes of scratch per lane (dynamic stack: %s)" % (kernel, private, dynamic)
        assert lds == 0, (kernel, lds)
