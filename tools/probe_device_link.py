"""Wall time of verifying the BN254 half of device proofs on the GPU (cg_device_link_verify_batch, csrc/devicelink.hip) under
a synthetic key in the mDL-like layout [COMMITTED, HIDDEN, COMMITTED, COMMITTED, REVEALED] with the device keys at inputs 2
and 3 and h_Q of 32 bytes.  Proofs come from the pure-Python prover of tests/device_link_vectors.py: --distinct of them (64:
one wave's worth, so that no two lanes of a wave walk the same table entries or take the same branches), repeated to the
batch size.  Every verdict must be CG_VERIFY_ACCEPT and every digest the prover's, before anything is timed.  Per size,
median of --reps calls after a warm-up: the call's wall time - it is synchronous and works on the handle's own stream, so
that covers the copies, four kernels per chunk and the stream synchronisation - and, of the run with the median wall time,
the HIP-event time of each kernel (cg_device_link_last_kernel_ms: an event pair around each).  Prints one JSON line.

    python tools/probe_device_link.py [--sizes 1,1024,16384] [--reps 7] [--distinct 64] [--out FILE]
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

KERNELS = ("k_dl_check", "k_dl_terms", "k_dl_sum", "k_dl_challenge")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,1024,16384")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import crescent_credentials_amd as cc
    import device_link_vectors as D
    import verify_vectors as V
    assert cc.lib().cg_init(0, None) == 0, cc.lib().cg_last_error()
    key = D.make_key([D.COMMITTED, D.HIDDEN, D.COMMITTED, D.COMMITTED, D.REVEALED], 2, 3, 0xDE71CE)
    pvk = cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(key.vk)))
    rng = random.Random(0x9B0BE)
    recs = [D.random_record(key, rng) for _ in range(a.distinct)]
    cols = [np.frombuffer(b, np.uint8).reshape(a.distinct, -1) for b in D.pack([D.record_bytes(key, r) for r in recs])]
    digests = np.stack([np.frombuffer(r.digest, np.uint8) for r in recs])
    res = {"layout": key.io, "h_len": 32, "distinct": a.distinct, "library": os.path.basename(cc.library_path()), "reps": a.reps, "sizes": {}}
    for n in [int(s) for s in a.sizes.split(",")]:
        idx = np.arange(n) % a.distinct
        arrays = [c[idx].reshape(-1).copy() for c in cols]
        call = lambda: cc.Groth16.device_link_verify_batch_packed(pvk, key.io, key.pos0, key.pos1, *arrays, h_len=32)
        verdicts, parts, e = call()                               # warm-up, buffer growth
        assert (verdicts == cc.CG_VERIFY_ACCEPT).all() and (parts == cc.CG_VERIFY_ACCEPT).all() and np.array_equal(e, digests[idx])
        runs = []
        for _ in range(a.reps):
            t = time.perf_counter()
            call()
            runs.append(((time.perf_counter() - t) * 1e3, pvk.device_link_last_kernel_ms()))
        runs.sort(key=lambda r: r[0])
        wall, ms = runs[len(runs) // 2]
        res["sizes"][str(n)] = {"median_ms": wall, "min_ms": runs[0][0], "spread_ms": runs[-1][0] - runs[0][0], "kernel_ms": dict(zip(KERNELS, ms)),
                                "kernels_ms": sum(ms), "per_s": n / (wall / 1e3)}
    pvk.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
