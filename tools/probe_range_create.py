"""Wall time of creating range proofs on the GPU (csrc/rangeproof.hip) at n_bits = 32 under a synthetic KZG key: the load
(host-built tables of 72 bases and their upload), cg_range_pk_add_bases, and the three calls cg_range_commit_batch,
cg_range_quotient_batch and cg_range_open_batch for batches of distinct openings with distinct random values (a
duplicated row would walk the same table entries in every wave).  Row 0 of every batch is checked byte for byte against
the restatement of tests/range_vectors.py.  The calls are synchronous and work on the handle's own stream, so what is
timed is the call itself: the copies, two kernels per chunk and the stream synchronisation; next to it the HIP-event
time of the two kernels (cg_range_pk_last_kernel_ms).  Prints one JSON line.

    python tools/probe_range_create.py [--n-bits 32] [--sizes 1,256,4096] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def _timed(fn, key, reps):
    """(median ms, min ms, polynomial-kernel ms, point-kernel ms of the median-most run)"""
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        runs.append(((time.perf_counter() - t) * 1e3,) + key.last_kernel_ms())
    runs.sort()
    mid = runs[len(runs) // 2]
    return {"median_ms": statistics.median(r[0] for r in runs), "min_ms": runs[0][0], "poly_kernel_ms": mid[1], "points_kernel_ms": mid[2]}


def _scalars(rng, count):
    """count canonical scalars: 32 random bytes with the top one below 0x30, the scalar modulus's"""
    a = rng.integers(0, 256, size=(count, 32), dtype=np.uint8)
    a[:, 31] %= 0x30
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-bits", type=int, default=32)
    ap.add_argument("--sizes", default="1,256,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import bn254_oracle as o
    import crescent_credentials_amd as cc
    import range_vectors as RV
    assert cc.lib().cg_init(0, None) == 0, cc.lib().cg_last_error()
    nb = a.n_bits
    K = RV.key(nb)
    bases = [RV.g1(0x1234567), RV.g1(0x89ABCDEF123)]
    t0 = time.perf_counter()
    key = cc.RangeProofKey(K.data, nb)
    load_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    slot = key.add_bases(*[o.g1_uncompressed(P) for P in bases])
    res = {"n_bits": nb, "library": os.path.basename(cc.library_path()), "load_ms": load_ms, "add_bases_ms": (time.perf_counter() - t0) * 1e3,
           "terms": {"commit": nb + 17, "quotient": 2 * nb + 7, "open": 4 * nb + 15}, "sizes": {}}
    rng = np.random.default_rng(2028)
    G = cc.Groth16
    val = lambda row: int.from_bytes(row.tobytes(), "little")
    for n in [int(s) for s in a.sizes.split(",")]:
        openings = _scalars(rng, 2 * n).reshape(n, 2, 32)
        openings[:, 0, max(nb // 8, 1):] = 0                           # m < 2^n_bits
        if nb < 8:
            openings[:, 0, 0] &= (1 << nb) - 1
        rand, c, rho = _scalars(rng, 18 * n).reshape(n, 18, 32), _scalars(rng, n), _scalars(rng, n)
        commit = lambda: G.range_commit_batch_packed(key, slot, openings, rand)
        quotient = lambda: G.range_quotient_batch_packed(key, openings, rand, c)
        opened = lambda: G.range_open_batch_packed(key, openings, rand, c, rho)
        got = commit(), quotient(), opened()                          # warm-up, buffer growth
        assert all((part[-1] == cc.CG_SHOW_MADE).all() for part in got)
        x = RV.prove(K, bases, val(openings[0, 0]), val(openings[0, 1]), [val(r) for r in rand[0]], 0, val(c[0]), val(rho[0]))
        for mine, want in zip((got[0][0], got[0][1], got[0][2]), RV.expected_commit(x)):
            assert mine[0].tobytes() == want
        for mine, want in zip(got[1][:2], RV.expected_quotient(x)):
            assert mine[0].tobytes() == want
        for mine, want in zip(got[2][:2], RV.expected_open(x)):
            assert mine[0].tobytes() == want
        t = {"commit": _timed(commit, key, a.reps), "quotient": _timed(quotient, key, a.reps), "open": _timed(opened, key, a.reps)}
        total = sum(v["median_ms"] for v in t.values())
        t["three_calls_median_ms"] = total
        t["range_proofs_per_s"] = n / (total / 1e3)
        res["sizes"][str(n)] = t
    key.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
