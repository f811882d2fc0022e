"""What pi2's public inputs cost on the GPU (cg_p256_tu_batch, cg_p256_rtu_batch, csrc/p256tu.hip): 64 distinct signed rows of
tests/p256_vectors.py repeated to the batch size, under a synthetic key whose only part in it is the handle.  Before anything
is timed every output byte and status of both calls must be the pure-Python oracle's.  Per size, in ONE run:

    tu, rtu     median wall ms of --reps synchronous calls after a warm-up, and of the run with the median wall time the
                HIP-event times of the three kernels (cg_p256_last_kernel_ms): the scalar stage, the terms, the finishing stage
    host        one thread of the g++ -O2 build of the same headers (tests/cpp/test_p256.cpp, `time tu` / `time rtu`): ns per
                row over --host-rows rows, times n

and the condition wall <= host / 16 (a host with 16 threads and no other work).  Registers, LDS and scratch per kernel are read
from the metadata of the library's gfx950 code object.  Prints one JSON line.

    python tools/probe_p256_tu.py [--sizes 1,1024,16384] [--reps 7] [--distinct 64] [--host-rows 256] [--out FILE]
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

KERNELS = ("scalars", "terms", "finish")


def timed(call, last_ms, reps):
    """median run of `reps` calls by wall time -> (all runs sorted, the median one)"""
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        runs.append(((time.perf_counter() - t) * 1e3, last_ms()))
    runs.sort(key=lambda r: r[0])
    return runs, runs[len(runs) // 2]


def host_ns_per_row(rows):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "test_p256")
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_p256.cpp")], check=True, capture_output=True)
        r = subprocess.run([exe], input="time tu %d\ntime rtu %d\n" % (rows, rows), capture_output=True, text=True, check=True)
        tu, rtu = r.stdout.split()
        return float(tu), float(rtu)


def kernel_resources(library):
    """VGPR, SGPR, LDS and scratch of the k_p256_* kernels, from the notes of the gfx950 code object"""
    readelf, objdump = "/opt/rocm/lib/llvm/bin/llvm-readelf", "/opt/rocm/lib/llvm/bin/llvm-objdump"
    out = {}
    with tempfile.TemporaryDirectory() as d:
        work = os.path.join(d, "lib.so")
        shutil.copy(library, work)
        subprocess.run([objdump, "--offloading", work], capture_output=True, text=True, check=True, cwd=d)
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([readelf, "--notes", os.path.join(d, f)], capture_output=True, text=True, check=True).stdout
            for blk in re.split(r"\n\s*- \.", notes):
                nm = re.search(r"\.name:\s+\S*?\d(k_p256_[a-z0-9_]+?)E", blk)
                if not nm or ".private_segment_fixed_size" not in blk:
                    continue
                field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                out[nm.group(1)] = {"vgpr": field("vgpr_count"), "sgpr": field("sgpr_count"), "lds": field("group_segment_fixed_size"),
                                    "scratch": field("private_segment_fixed_size")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,1024,16384")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--host-rows", type=int, default=256)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import crescent_credentials_amd as cc
    import device_link_vectors as D
    import p256_vectors as PV
    import verify_vectors as V
    assert cc.lib().cg_init(0, None) == 0, cc.lib().cg_last_error()
    key = D.make_key([D.COMMITTED, D.HIDDEN, D.COMMITTED, D.COMMITTED, D.REVEALED], 2, 3, 0xDE71CE)
    pvk = cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(key.vk)))
    rows = PV.signed_rows(0x9B0BE, a.distinct)
    want = [PV.compute_rtu(*row) for row in rows]
    assert all(w[0] == PV.MADE for w in want)
    col = lambda items: np.stack([np.frombuffer(b, np.uint8) for b in items])
    qs, sigs, dgs = (col([row[j] for row in rows]) for j in range(3))
    rs, ts, us = (col([w[j] for w in want]) for j in (1, 2, 3))
    host_tu, host_rtu = host_ns_per_row(a.host_rows)
    res = {"distinct": a.distinct, "library": os.path.basename(cc.library_path()), "reps": a.reps, "host_ns_per_row": {"tu": host_tu, "rtu": host_rtu},
           "host_rows_timed": a.host_rows, "kernels": kernel_resources(cc.library_path()), "sizes": {}}
    G = cc.Groth16
    for n in [int(x) for x in a.sizes.split(",")]:
        idx = np.arange(n) % a.distinct
        q, sig, dg, r_in = (x[idx].reshape(-1).copy() for x in (qs, sigs, dgs, rs))
        rtu = lambda: G.p256_rtu_batch(pvk, q, sig, dg)
        tu = lambda: G.p256_tu_batch(pvk, r_in, dg)
        r, t, u, status = rtu()                                    # warm-up, buffer growth, and the bytes
        assert (status == cc.CG_SHOW_MADE).all() and np.array_equal(r, rs[idx]) and np.array_equal(t, ts[idx]) and np.array_equal(u, us[idx])
        t, u, status = tu()
        assert (status == cc.CG_SHOW_MADE).all() and np.array_equal(t, ts[idx]) and np.array_equal(u, us[idx])
        entry = {}
        for name, call, host_ns in (("tu", tu, host_tu), ("rtu", rtu, host_rtu)):
            runs, (wall, ms) = timed(call, pvk.p256_last_kernel_ms, a.reps)
            host_ms = host_ns * n / 1e6
            entry[name] = {"median_ms": wall, "min_ms": runs[0][0], "spread_ms": runs[-1][0] - runs[0][0], "kernel_ms": dict(zip(KERNELS, ms[:3])),
                           "per_s": n / (wall / 1e3), "host_one_thread_ms": host_ms,
                           "condition": {"wall_ms": wall, "sixteenth_of_host_ms": host_ms / 16, "holds": wall <= host_ms / 16,
                                         "factor": host_ms / 16 / wall}}
        res["sizes"][str(n)] = entry
    pvk.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
