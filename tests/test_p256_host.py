"""csrc/fq256.hpp, csrc/p256.hpp and the two functions csrc/fp256.hpp gained for them, on the HOST (g++ build of
tests/cpp/test_p256.cpp) against Python integers and tests/p256_vectors.py: the scalar field at n's edges - (n - 1) + (n - 1)
and (n - 1)^2 among them, where the sum and the Montgomery accumulator pass 2^256 -, the inversions, the complete addition on
equal, opposite and identity operands, k G by the table walk and k P by the windowed chain, the table's first and last rows,
whole rows of compute_TU and compute_RTU with every status, and the rows of tests/steer_vectors.py, which are steered to the
rare branch of both fields' reductions and to the protocol's edges (R.x in [n, p), digests that are 0 mod n, structured scalars).  The same program, built with the address and
undefined-behaviour sanitizers, answers the same requests on its own.  Then, without running anything: the kernels of csrc/p256tu.hip
declare no private segment.  Pure CPU.

Doubling a point of the form (x, 0) is not tested: the group has odd order, so it has no point of order two and the curve
no point with y = 0."""
import os
import random
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
import p256_vectors as V
import steer_vectors as S

P, N, G = V.P, V.N, V.G
SRC = os.path.join(ROOT, "tests", "cpp", "test_p256.cpp")
EDGES = [0, 1, 2, N - 1, N - 2, 1 << 255, (1 << 255) + 1, (1 << 255) - 1, 1 << 224, (1 << 32) - 1]
ZERO_WINDOWS = (0xAB << 248) | (0x0F << 120) | 0x10      # most 8-bit and 4-bit windows are zero
SCALARS = [0, 1, 2, N - 1, N - 2, 1 << 255, (1 << 256) - 1, int("f" * 56, 16), ZERO_WINDOWS]      # 2^256 - 1: every window full; Python takes it mod n
be = lambda v: int(v).to_bytes(32, "big").hex()
pt = lambda p: V.point_bytes(p).hex()


def ask_all(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = r.stdout.split()
    assert len(out) == len(lines) and "ERR" not in out, r.stdout[-2000:]
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("p256") / "test_p256")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", path, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def compare(exe, lines, want):
    got = ask_all(exe, lines)
    for line, g, w in zip(lines, got, want):
        assert g == w, line[:120]


# ---- the two fields -----------------------------------------------------------------------------------------------------------
def field_lines(n_random, n_inv):
    rng = random.Random(0xF0256)
    pairs = [(a, b) for a in EDGES for b in EDGES] + [(rng.randrange(N), rng.randrange(N)) for _ in range(n_random)]
    assert (N - 1, N - 1) in pairs
    lines, want = [], []
    for a, b in pairs:
        lines += ["qadd %s %s" % (be(a), be(b)), "qsub %s %s" % (be(a), be(b)), "qmul %s %s" % (be(a), be(b))]
        want += [be((a + b) % N), be((a - b) % N), be(a * b % N)]
    for a in [1, 2, N - 1, N - 2, 1 << 255] + [rng.randrange(1, N) for _ in range(n_inv - 5)]:
        lines.append("qinv " + be(a))
        want.append(be(pow(a, -1, N)))
    lines.append("qinv " + be(0))
    want.append(be(0))
    for v, ok in ((0, 1), (N - 1, 1), (N, 0), (N + 1, 0), ((1 << 256) - 1, 0), (1 << 255, 1), (N - (1 << 128), 1), (N + (1 << 128), 0)):
        lines.append("qbelow " + be(v))
        want.append(str(ok))
    lines.append("qconsts")
    want.append("1")
    for a in [1, 2, P - 1, P - 2, 1 << 255, (1 << 96) - 1] + [rng.randrange(1, P) for _ in range(n_inv - 6)]:
        lines += ["pinv " + be(a), "pneg " + be(a)]
        want += [be(pow(a, -1, P)), be(-a % P)]
    lines += ["pinv " + be(0), "pneg " + be(0)]
    want += [be(0), be(0)]
    return lines, want


def test_scalar_field_at_the_edges_and_on_random_pairs_and_both_inversions(exe):
    lines, want = field_lines(10000, 64)
    compare(exe, lines, want)
    assert 2 * (N - 1) >= 1 << 256                                             # the sum Fp<P> cannot hold


# ---- the group -----------------------------------------------------------------------------------------------------------------
def group_lines(n_random):
    rng = random.Random(0x6256)
    A, B = V.mul(rng.randrange(N), G), V.mul(rng.randrange(N), G)
    lines, want = [], []
    for p, q in ((A, A), (A, V.neg(A)), (A, None), (None, A), (None, None), (A, B), (G, G), (G, V.neg(G))):
        lines.append("gadd %s %s" % (pt(p), pt(q)))
        want.append(pt(V.add(p, q)))
    for p, q in ((A, A), (A, V.neg(A)), (None, A), (A, B)):
        lines.append("gmixed %s %s" % (pt(p), pt(q)))
        want.append(pt(V.add(p, q)))
    for p, ok in ((G, 1), ((G[0], G[1] + 1), 0), ((P, G[1]), 0), (((1 << 256) - 1, G[1]), 0), ((0, 0), 0), (A, 1)):
        lines.append("oncurve " + be(p[0]) + be(p[1]))
        want.append(str(ok))
    for k in SCALARS + [rng.randrange(1 << 256) for _ in range(n_random)]:
        lines += ["walk " + be(k), "chain %s %s" % (be(k), pt(A))]
        want += [pt(V.mul(k, G)), pt(V.mul(k, A))]
    return lines, want


def test_complete_addition_on_every_case_and_scalar_products_against_python(exe):
    lines, want = group_lines(64)
    assert sum(w == pt(None) for w in want) >= 5                               # P + (-P), O + O, 0 G and 0 P among them
    compare(exe, lines, want)


def test_first_and_last_rows_of_the_table(exe):
    first, last = ask_all(exe, ["tabrow 0", "tabrow 31"])
    for row, base in ((first, G), (last, V.mul(1 << 248, G))):
        assert len(row) == 255 * 128
        acc = None
        for d in range(255):
            acc = V.add(acc, base)
            assert row[128 * d:128 * d + 128] == pt(acc), d


# ---- compute_TU and compute_RTU ---------------------------------------------------------------------------------------------------
def row_lines(n_random):
    lines, want = [], []
    rows = V.signed_rows(0x7256, n_random) + [V.coincident_row(0x1234567, 0x89ABCDE), V.coincident_row(0x1234567, 0x89ABCDE, opposite=True)]
    for q, sig, dg in rows:
        st, r, t, u = V.compute_rtu(q, sig, dg)
        lines.append("rtu %s %s %s" % (q.hex(), sig.hex(), dg.hex()))
        want.append("%d%s%s%s" % (st, r.hex(), t.hex(), u.hex()))
        if st == V.MADE:
            st2, t2, u2 = V.compute_tu(r, dg)
            assert (st2, t2, u2) == (V.MADE, t, u)
            lines.append("tu %s %s" % (r.hex(), dg.hex()))
            want.append("1%s%s" % (t.hex(), u.hex()))
    q, sig, dg = rows[0]
    r = V.compute_rtu(q, sig, dg)[1]
    bad_y = r[:32] + V.be(int.from_bytes(r[32:], "big") + 1)
    for r_xy, d in ((bad_y, dg), (V.be(P) + r[32:], dg), (r, bytes(32)), (r, V.be(N + 5)), (r, V.be(N))):
        st, t, u = V.compute_tu(r_xy, d)
        lines.append("tu %s %s" % (r_xy.hex(), d.hex()))
        want.append("%d%s%s" % (st, t.hex(), u.hex()))
    for sig2 in (V.be(0) + sig[32:], V.be(N) + sig[32:], sig[:32] + V.be(0), sig[:32] + V.be(N), V.be(int.from_bytes(sig[:32], "big") - 1) + sig[32:]):
        st, r2, t, u = V.compute_rtu(q, sig2, dg)
        lines.append("rtu %s %s %s" % (q.hex(), sig2.hex(), dg.hex()))
        want.append("%d%s%s%s" % (st, r2.hex(), t.hex(), u.hex()))
    return lines, want


def test_whole_rows_with_every_status(exe):
    lines, want = row_lines(8)
    assert {w[0] for w in want} == {"1", "2", "3"}
    compare(exe, lines, want)


# ---- rows steered to the rare branches (tests/steer_vectors.py; tests/test_steer_vectors_cpu.py shows that each hits its case) --------
def steered_lines(family, per_family=None):
    """the family's vectors as `tu` and `rtu` requests with the oracle's answers; per_family: only every n-th"""
    lines, want = [], []
    for v in S.p256_families()[family][::per_family or 1]:
        lines.append(v.kind + " " + " ".join(a.hex() for a in v.args))
        w = S.expected(v)
        want.append(str(w[0]) + "".join(b.hex() for b in w[1:]))
    return lines, want


@pytest.mark.parametrize("family", [name for name, _ in S.P256_FAMILIES])
def test_steered_rows_byte_for_byte(exe, family):
    lines, want = steered_lines(family)
    assert len(lines) == S.P256_COUNTS[family]
    compare(exe, lines, want)


def test_steered_scalars_through_the_scalar_field_alone(exe):
    """d, s and r whose q256_to_mont takes the rare branch, one operation each: x + 0, x * 1 and x^-1"""
    xs = [S.facts(v)["scalar"] for v in S.p256_families()["entry_points"] if S.facts(v)["site"] in "dsr"]
    assert len(xs) == 10 and all(S.from_words_hits(x, N) for x in xs)
    lines, want = [], []
    for x in xs:
        lines += ["qadd %s %s" % (be(x), be(0)), "qmul %s %s" % (be(x), be(1)), "qinv " + be(x), "qadd %s %s" % (be(x), be(N - x))]
        want += [be(x), be(x), be(pow(x, -1, N)), be(0)]
    # sums of representations in [n, 2^256): a + b = delta 2^-256 with the representations adding up to n + delta
    for delta in (0, 1, (1 << 256) - 1 - N):
        a = 0x1234567 << 200
        b = (S.unmont(delta, N) - a) % N
        assert S.mont(a, N) + S.mont(b, N) == N + delta
        lines.append("qadd %s %s" % (be(a), be(b)))
        want.append(be((a + b) % N))
    compare(exe, lines, want)


def test_sanitized_build_answers_the_same(tmp_path):
    path = str(tmp_path / "test_p256_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", path, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines, want = field_lines(300, 8)
    for a, b in [group_lines(2), row_lines(2)] + [steered_lines(name, 7) for name, _ in S.P256_FAMILIES]:
        lines, want = lines + a, want + b
    assert ask_all(path, lines + ["tabrow 31"])[:-1] == want


# ---- the code objects, without a GPU ---------------------------------------------------------------------------------------------
def test_p256_kernels_declare_no_private_segment(cc, tmp_path):
    """A chain's table is in global memory, scalars and digits are read through pointers, and no per-lane array is indexed by
    a run-time value: no scratch.  Kernel metadata of the shipped gfx950 code objects only: nothing runs."""
    readelf, objdump = "/opt/rocm/lib/llvm/bin/llvm-readelf", "/opt/rocm/lib/llvm/bin/llvm-objdump"
    assert os.path.exists(readelf) and os.path.exists(objdump)
    work = os.path.join(str(tmp_path), "lib.so")
    shutil.copy(cc.library_path(), work)
    subprocess.run([objdump, "--offloading", work], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    want = {"k_p256_tu_scalars", "k_p256_rtu_scalars", "k_p256_terms", "k_p256_tu_finish", "k_p256_rtu_finish"}
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
                for kernel in re.findall(r"\d(k_p256_[a-z0-9_]+?)E", nm.group(1)):
                    seen[kernel] = (int(ps.group(1)), dyn.group(1) if dyn else "false", int(lds.group(1)), int(spill.group(1)) if spill else 0)
    assert set(seen) == want, seen
    for kernel, (private, dynamic, lds, spill) in seen.items():
        assert private == 0 and dynamic == "false" and spill == 0, "%s: %d bytes of scratch per lane (dynamic stack: %s)" % (kernel, private, dynamic)
        assert lds == 0, (kernel, lds)
