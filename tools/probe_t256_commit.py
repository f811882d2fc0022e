"""What committing pi2's witness costs on the GPU (cg_hyrax_commit_batch, csrc/t256commit.hip): batches of distinct proofs of
2^num_vars scalars each over a set of known multiples of G (tests/t256_vectors.py), with uniform scalars and with bench.py's
wire mix (56 % zero, 34 % one, 10 % uniform).  Row 0 of every batch is checked byte for byte against the oracle's closed form
before anything is timed.

    wall        the call: copies, three kernels per chunk, the stream synchronisation (median and minimum of --reps)
    kernels     HIP-event times of the check and of the group stage (cg_t256_commit_last_kernel_ms), and the lanes per row
    walk rate   mixed additions per second of the group stage: the non-zero bytes of the call's scalars and blinds over its
                time - the butterfly and the normalisation are inside that time
    host        one thread of the g++ -O2 build of the same headers (tests/cpp/test_t256.cpp, `time`): ns per row, and what the
                batch would take on sixteen such threads
    resources   VGPRs, LDS, scratch of the k_t256_* kernels from the code object's notes; the bytes of the set's tables

    python tools/probe_t256_commit.py [--num-vars 13,15] [--proofs 64,1024] [--reps 3] [--host-rows 32] [--out FILE]
"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def scalars(rng, count, mix):
    """count x 32 bytes little-endian below 2^255 < q; mix: 56 % zero, 34 % one, the rest uniform"""
    a = rng.integers(0, 256, size=(count, 32), dtype=np.uint8)
    a[:, 31] &= 0x7F
    if mix:
        u = rng.random(count)
        a[u < 0.90] = 0
        a[(u >= 0.56) & (u < 0.90), 0] = 1
    return a


def host_ns_per_row(n_gens, rows, mix):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "test_t256")
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_t256.cpp")], check=True, capture_output=True)
        out = subprocess.run([exe], input="time %d %d %s\n" % (n_gens, rows, "mix" if mix else "uniform"), capture_output=True, text=True, check=True)
        return float(out.stdout.split()[0])


def kernel_resources(lib_path):
    """VGPR, SGPR, LDS and scratch of the k_t256_* kernels, from the notes of the gfx950 code object"""
    readelf, objdump = "/opt/rocm/lib/llvm/bin/llvm-readelf", "/opt/rocm/lib/llvm/bin/llvm-objdump"
    res = {}
    if not (os.path.exists(readelf) and os.path.exists(objdump)):
        return res
    with tempfile.TemporaryDirectory() as d:
        work = os.path.join(d, "lib.so")
        shutil.copy(lib_path, work)
        subprocess.run([objdump, "--offloading", work], capture_output=True, text=True, check=True, cwd=d)
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([readelf, "--notes", os.path.join(d, f)], capture_output=True, text=True, check=True).stdout
            for blk in re.split(r"\n\s*- \.", notes):
                nm = re.search(r"\.name:\s+\S*?\d(k_t256_[a-z0-9_]+?)E", blk)
                if nm:
                    get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
                    res[nm.group(1)] = {"vgprs": get("vgpr_count"), "sgprs": get("sgpr_count"), "lds_bytes": get("group_segment_fixed_size"),
                                        "scratch_bytes": get("private_segment_fixed_size")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-vars", default="13,15")
    ap.add_argument("--proofs", default="64,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=32)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import crescent_credentials_amd as cc
    import t256_vectors as V
    assert cc.lib().cg_init(0, None) == 0, cc.lib().cg_last_error()
    res = {"library": os.path.basename(cc.library_path()), "kernels": kernel_resources(cc.library_path()), "shapes": {}}
    rng = np.random.default_rng(2256)
    val = lambda row: int.from_bytes(row.tobytes(), "little")
    for nv in [int(s) for s in a.num_vars.split(",")]:
        L, R = V.factored_lens(nv)
        gens = V.make_gens(0x9E0 + nv, R)
        t0 = time.perf_counter()
        handle = cc.T256Gens(gens.g_xy, gens.h_xy)
        shape = {"L": L, "R": R, "load_ms": (time.perf_counter() - t0) * 1e3, "table_bytes": handle.table_bytes, "runs": {}}
        for mix in (False, True):
            name = "mix" if mix else "uniform"
            host_ns = host_ns_per_row(R, a.host_rows, mix)
            for n in [int(s) for s in a.proofs.split(",")]:
                vars_, blinds = scalars(rng, n * L * R, mix), scalars(rng, n * L, False)
                call = lambda: handle.hyrax_commit_batch(nv, vars_, blinds)
                out, status = call()                                   # warm-up, buffer growth
                assert (status == cc.CG_SHOW_MADE).all()
                want = gens.commit([val(r) for r in vars_[:R]], val(blinds[0]))
                assert out[0, 0].tobytes() == want[1], "row 0 differs from the oracle"
                runs = []
                for _ in range(a.reps):
                    t = time.perf_counter()
                    call()
                    runs.append(((time.perf_counter() - t) * 1e3,) + handle.commit_last_kernel_ms())
                runs.sort()
                mid = runs[len(runs) // 2]
                adds = int(np.count_nonzero(vars_)) + int(np.count_nonzero(blinds))
                rows = n * L
                shape["runs"]["%s_%d" % (name, n)] = {
                    "rows": rows, "scalar_bytes": int(vars_.nbytes), "wall_median_ms": statistics.median(r[0] for r in runs), "wall_min_ms": runs[0][0],
                    "check_kernel_ms": mid[1], "group_kernel_ms": mid[2], "lanes_per_row": mid[3], "mixed_additions": adds,
                    "mixed_additions_per_s": adds / (mid[2] / 1e3), "host_ns_per_row": host_ns, "host_one_thread_ms": host_ns * rows / 1e6,
                    "host_sixteen_threads_ms": host_ns * rows / 16e6}
                del vars_, blinds
        handle.close()
        res["shapes"][str(nv)] = shape
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
