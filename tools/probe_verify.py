"""Wall time of cg_verify_batch (Groth16 verification on the GPU, csrc/verify.hip) at a synthetic key with ell public
inputs for several batch sizes: one valid proof duplicated n times, verdicts checked.  Prints one JSON line; run it under
`rocprofv3 --kernel-trace --stats -- python tools/probe_verify.py` for the per-kernel times.

    python tools/probe_verify.py [--ell 26] [--sizes 1,64,1024,16384] [--reps 5] [--latency] [--out FILE]

--latency adds, per size, both arrangements of the pairing stage (cg_pvk_set_latency_mode) alternated in this process.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def _alternated(cc, pvk, ib, pb, reps):
    """--latency: the wide and the latency arrangement on the same handle, alternated call by call after a warm-up of each;
    per arrangement the median wall time and that call's (group, pairing) HIP-event times"""
    runs = {False: [], True: []}
    for mode in (False, True):
        pvk.set_latency(mode)
        assert (cc.Groth16.verify_batch(pvk, ib, pb) == cc.CG_VERIFY_ACCEPT).all()
    for _ in range(reps):
        for mode in (False, True):
            pvk.set_latency(mode)
            t = time.perf_counter()
            cc.Groth16.verify_batch(pvk, ib, pb)
            runs[mode].append(((time.perf_counter() - t) * 1e3,) + pvk.last_kernel_ms())
    pvk.set_latency(False)
    out = {}
    for mode, name in ((False, "wide"), (True, "latency")):
        r = sorted(runs[mode])
        mid = r[len(r) // 2]
        out[name] = {"median_ms": statistics.median(x[0] for x in r), "min_ms": r[0][0], "group_kernel_ms": mid[1], "pairing_kernel_ms": mid[2]}
    out["wide_over_latency"] = out["wide"]["median_ms"] / out["latency"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latency", action="store_true", help="also time both arrangements of the pairing stage, alternated")
    ap.add_argument("--ell", type=int, default=26)
    ap.add_argument("--sizes", default="1,64,1024,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import crescent_credentials_amd as cc
    import verify_vectors as V
    assert cc.lib().cg_init(0, None) == 0, cc.lib().cg_last_error()
    rng = random.Random(2026)
    R = V.R
    sc = tuple(rng.randrange(1, R) for _ in range(4)) + ([rng.randrange(R) for _ in range(a.ell + 1)],)
    xs = [rng.randrange(R) for _ in range(a.ell)]
    proof = V.proof_bytes(V.synthetic_proof(sc, xs, a=rng.randrange(1, R), b=rng.randrange(1, R)))
    vkb = V.vk_bytes(V.synthetic_vk(*sc[:4], sc[4]))
    t0 = time.perf_counter()
    pvk_bytes = cc.Groth16.prepare_verifying_key(vkb)
    t1 = time.perf_counter()
    pvk = cc.PreparedVerifyingKey(pvk_bytes)
    t2 = time.perf_counter()
    res = {"ell": a.ell, "prepare_verifying_key_ms": (t1 - t0) * 1e3, "pvk_load_ms": (t2 - t1) * 1e3, "sizes": {}}
    ib1 = np.frombuffer(V.inputs_bytes(xs), np.uint8)
    pb1 = np.frombuffer(proof, np.uint8)
    for n in [int(s) for s in a.sizes.split(",")]:
        ib, pb = np.tile(ib1, n), np.tile(pb1, n)
        v = cc.Groth16.verify_batch(pvk, ib, pb)            # warm-up (and buffer growth)
        assert (v == cc.CG_VERIFY_ACCEPT).all()
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            cc.Groth16.verify_batch(pvk, ib, pb)
            ts.append(time.perf_counter() - t)
        med = statistics.median(ts)
        res["sizes"][str(n)] = {"median_ms": med * 1e3, "min_ms": min(ts) * 1e3, "proofs_per_s": n / med}
        if a.latency:
            res["sizes"][str(n)].update(_alternated(cc, pvk, ib, pb, a.reps))
    s = res["sizes"]
    if "1" in s and "16384" in s:
        res["rate_16384_over_rate_1"] = s["16384"]["proofs_per_s"] / s["1"]["proofs_per_s"]
    pvk.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
