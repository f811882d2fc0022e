"""The entries built on csrc/merlin.hpp, as far as they go without a GPU: cg_dlog_challenge_batch (host only) against the
pure-Python Merlin of tests/merlin_vectors.py on real curve points, its contexts, threads and refusals; the three entries
declared, exported and bound; the null handle of the two GPU entries; and, from the shipped gfx950 code objects' metadata,
that the challenge kernels declare no private segment.  (A handle needs a device: the null arrays under a handle are in
tests/test_gpu_range_one_call.py.)"""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import merlin_vectors as MV
import range_vectors as RV

o = RV.o
R, Q = o.R, o.Q
INVALID_ARGUMENT = -1
unc, cmp = o.g1_uncompressed, o.g1_compressed


def points(rng, n):
    return [RV.g1(rng.randrange(1, R)) for _ in range(n)]


def batch(rng, shape, n):
    """the shared bases and, per showing, k and y of a DLogPoK of this shape: real points, infinity among the y"""
    bases = points(rng, sum(shape))
    ks = [points(rng, len(shape)) for _ in range(n)]
    ys = [points(rng, len(shape)) for _ in range(n)]
    if n > 2:
        ys[2][0] = None
    return bases, ks, ys


def want(context, shape, bases, k, y):
    st, at = [], 0
    for i, nb in enumerate(shape):
        st.append(([cmp(B) for B in bases[at:at + nb]], cmp(k[i]), cmp(y[i])))
        at += nb
    return MV.to_scalar_bytes(MV.dlog_challenge(context, st))


def call(cc, shape, bases, ks, ys, **kw):
    return cc.Groth16.dlog_challenge_batch(
        shape, b"".join(unc(B) for B in bases), b"".join(cmp(P) for k in ks for P in k),
        b"".join(unc(P) for y in ys for P in y[:-1]) if len(shape) > 1 else None, b"".join(unc(y[-1]) for y in ys), **kw)


def test_known_answers_through_the_entry(cc):
    """KATs 3-5 fix the framing on arbitrary bytes (tests/test_merlin_host.py); here the same shapes and contexts on curve
    points, which the entry compresses itself"""
    MV.self_check()
    rng = random.Random(50)
    for context, shape, _ in MV.KAT_DLOG:
        bases, ks, ys = batch(rng, shape, 3)
        got = call(cc, shape, bases, ks, ys, context=context)
        assert got.shape == (3, 32)
        for i in range(3):
            assert got[i].tobytes() == want(context, shape, bases, ks[i], ys[i]), (shape, i)
            assert got[i, 31] == 0


def test_none_and_the_empty_context_are_one_transcript(cc):
    rng = random.Random(51)
    bases, ks, ys = batch(rng, [2, 4], 1)
    assert call(cc, [2, 4], bases, ks, ys, context=None).tobytes() == call(cc, [2, 4], bases, ks, ys, context=b"").tobytes()


def test_a_context_per_showing_through_the_stride(cc):
    rng = random.Random(52)
    shape = [2, 3]
    bases, ks, ys = batch(rng, shape, 4)
    ctx = [bytes(rng.randrange(256) for _ in range(24)) for _ in range(4)]
    got = call(cc, shape, bases, ks, ys, context=b"".join(ctx), context_stride=24)
    assert [got[i].tobytes() for i in range(4)] == [want(ctx[i], shape, bases, ks[i], ys[i]) for i in range(4)]
    # a context shorter than the stride: the first 10 bytes of each slot
    got = call(cc, shape, bases, ks, ys, context=b"".join(ctx), context_len=10, context_stride=24)
    assert [got[i].tobytes() for i in range(4)] == [want(ctx[i][:10], shape, bases, ks[i], ys[i]) for i in range(4)]
    L = cc.lib()
    buf = (ctypes.c_uint8 * 4096)()
    nb = (ctypes.c_uint32 * 2)(2, 3)
    assert L.cg_dlog_challenge_batch(buf, 24, 10, 2, nb, buf, buf, buf, buf, 1, buf) == INVALID_ARGUMENT     # stride < length
    assert b"stride" in L.cg_last_error()


def test_a_batch_over_several_host_threads(cc):
    rng = random.Random(53)
    shape = [2, 2, 5]
    bases, ks, ys = batch(rng, shape, 33)
    got = call(cc, shape, bases, ks, ys, context=b"presentation")
    assert [got[i].tobytes() for i in range(33)] == [want(b"presentation", shape, bases, ks[i], ys[i]) for i in range(33)]


def test_one_statement_and_no_showings(cc):
    rng = random.Random(54)
    bases, ks, ys = batch(rng, [3], 2)
    got = call(cc, [3], bases, ks, ys)
    assert [got[i].tobytes() for i in range(2)] == [want(None, [3], bases, ks[i], ys[i]) for i in range(2)]
    L = cc.lib()
    nb = (ctypes.c_uint32 * 1)(3)
    assert L.cg_dlog_challenge_batch(None, 0, 0, 1, nb, b"".join(unc(B) for B in bases), None, None, None, 0, None) == 0       # n = 0
    assert call(cc, [3], bases, [], []).shape == (0, 32)


def test_a_coordinate_not_below_q_is_refused_with_nothing_written(cc):
    rng = random.Random(55)
    shape = [2, 2]
    bases, ks, ys = batch(rng, shape, 9)
    L = cc.lib()
    nb = (ctypes.c_uint32 * 2)(*shape)
    bb, kb = b"".join(unc(B) for B in bases), b"".join(cmp(P) for k in ks for P in k)
    head, last = bytearray(b"".join(unc(y[0]) for y in ys)), bytearray(b"".join(unc(y[1]) for y in ys))

    def run(bb, head, last):
        out = np.full(9 * 32, 0xAB, np.uint8)
        rc = L.cg_dlog_challenge_batch(None, 0, 0, 2, nb, bytes(bb), kb, bytes(head), bytes(last), 9, out.ctypes.data)
        return rc, out, L.cg_last_error()

    rc, out, _ = run(bb, head, last)
    assert rc == 0 and not (out == 0xAB).all()
    bad = bytearray(last)
    bad[64 * 6:64 * 6 + 32] = RV.fe(Q)                                           # x = q in showing 6's y_last
    rc, out, msg = run(bb, head, bad)
    assert rc == INVALID_ARGUMENT and b"showing 6" in msg and (out == 0xAB).all()
    bad = bytearray(head)
    bad[64 * 4 + 32:64 * 4 + 64] = RV.fe(Q + 1)                                  # y > q in showing 4's y_head
    rc, out, msg = run(bb, bad, last)
    assert rc == INVALID_ARGUMENT and b"showing 4" in msg and (out == 0xAB).all()
    bad = bytearray(last)
    bad[64 * 8 + 63] |= 0xC0                                                     # both flags
    rc, out, msg = run(bb, head, bad)
    assert rc == INVALID_ARGUMENT and b"showing 8" in msg and (out == 0xAB).all()
    bad = bytearray(bb)
    bad[64 * 3:64 * 3 + 32] = RV.fe(Q)
    rc, out, msg = run(bad, head, last)
    assert rc == INVALID_ARGUMENT and b"base 3" in msg and (out == 0xAB).all()
    # a point off the curve is not this entry's business: it is compressed as its bytes stand
    off = bytearray(last)
    off[0] ^= 1
    rc, out, _ = run(bb, head, off)
    assert rc == 0
    # null arrays and an empty proof of knowledge
    assert L.cg_dlog_challenge_batch(None, 0, 0, 2, nb, bb, None, bytes(head), bytes(last), 9, out.ctypes.data) == INVALID_ARGUMENT
    assert L.cg_dlog_challenge_batch(None, 0, 0, 2, nb, bb, kb, None, bytes(last), 9, out.ctypes.data) == INVALID_ARGUMENT
    assert L.cg_dlog_challenge_batch(None, 5, 0, 2, nb, bb, kb, bytes(head), bytes(last), 9, out.ctypes.data) == INVALID_ARGUMENT
    assert L.cg_dlog_challenge_batch(None, 0, 0, 0, nb, bb, kb, bytes(head), bytes(last), 9, out.ctypes.data) == INVALID_ARGUMENT


def test_the_gpu_entries_report_a_null_handle_before_any_hip_call(cc):
    L = cc.lib()
    buf = (ctypes.c_uint8 * 2048)()
    for n in (0, 1):
        assert L.cg_range_prove_batch(None, 0, buf, buf, buf, n, *([buf] * 9)) == INVALID_ARGUMENT
        assert b"null" in L.cg_last_error()
        assert L.cg_range_verify_proofs_batch(None, 0, *([buf] * 9), n, buf) == INVALID_ARGUMENT
        assert b"null" in L.cg_last_error()


def test_entries_are_declared_exported_and_bound(cc):
    from crescent_credentials_amd import api
    hdr = open(os.path.join(ROOT, "include", "crescent_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "sys.rs")).read()
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "lib.rs")).read()
    L = ctypes.CDLL(cc.library_path())
    for name, n_args in (("cg_range_prove_batch", 15), ("cg_range_verify_proofs_batch", 13), ("cg_dlog_challenge_batch", 11)):
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert hasattr(L, name) and len(api._SIGNATURES[name][1]) == n_args
        assert re.search(r"pub fn %s\s*\(" % name, sys_rs), name
        assert "sys::%s" % name in lib_rs, name
        assert code.index("cg_range_verify_batch") < code.index(name)            # after the entries they complete
    for f in (cc.Groth16.prove_range_batch, cc.Groth16.verify_range_proofs, cc.Groth16.dlog_challenge_batch,
              cc.Groth16.range_prove_batch_packed, cc.Groth16.range_verify_proofs_batch_packed, cc.Groth16.show_dlog_challenges):
        assert callable(f)
    assert "transcript.hip" in open(os.path.join(ROOT, "crescent-credentials_amd", "build.py")).read()


def test_challenge_kernels_declare_no_private_segment(cc, tmp_path):
    """A sponge indexed by a run-time position goes to scratch if it is a per-lane array; csrc/merlin.hpp keeps it in LDS.
    Kernel metadata of the shipped gfx950 code objects only: nothing runs."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    assert os.path.exists(readelf) and os.path.exists(objdump)
    work = os.path.join(str(tmp_path), "lib.so")
    shutil.copy(cc.library_path(), work)
    subprocess.run([objdump, "--offloading", work], capture_output=True, text=True, check=True, cwd=str(tmp_path))
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
                for kernel in ("k_range_challenge_c", "k_range_challenge_rho", "k_rv_challenges", "k_rv_challenge_dleq"):
                    if re.search(r"\d%s[A-Z]" % kernel, nm.group(1)):
                        seen[kernel] = (int(ps.group(1)), dyn.group(1) if dyn else "false", int(lds.group(1)))
    assert sorted(seen) == ["k_range_challenge_c", "k_range_challenge_rho", "k_rv_challenge_dleq", "k_rv_challenges"], seen
    for kernel, (private, dynamic, lds) in seen.items():
        assert private == 0 and dynamic == "false", "%s: %d bytes of scratch per lane (dynamic stack: %s)" % (kernel, private, dynamic)
        assert lds == 64 * 200, (kernel, lds)                                    # the sponges of one wave of lanes
