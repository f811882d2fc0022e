"""Wall time of creating the BN254 half of device proofs on the GPU (cg_device_link_prove_batch, csrc/devicelinkmake.hip), and
beside it of verifying the same proofs (cg_device_link_verify_batch) in the same run, under the key, the layout and the 64
distinct records of tools/probe_device_link.py: the mDL-like layout [COMMITTED, HIDDEN, COMMITTED, COMMITTED, REVEALED] with the
device keys at inputs 2 and 3, h_Q of 32 bytes, and the scalars drawn in the order tests/device_link_vectors.py's
random_record draws them from the same seed.  Every output row of the maker must be the pure-Python prover's and every verdict
on them CG_VERIFY_ACCEPT before anything is timed.  Per size, median of --reps calls after a warm-up: the call's wall time - it
is synchronous and works on the handle's own stream, so that covers the copies, six kernels per chunk and the stream
synchronisation - and, of the run with the median wall time, the HIP-event time of each kernel
(cg_device_link_prove_last_kernel_ms).  Prints one JSON line.

    python tools/probe_device_link_create.py [--sizes 1,1024,16384] [--reps 7] [--distinct 64] [--out FILE]
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

KERNELS = ("k_dlm_check", "k_dlm_terms", "k_dlm_sum", "k_dlm_pi0", "k_dlm_lhs1", "k_dlm_pi1")
VERIFY_KERNELS = ("k_dl_check", "k_dl_terms", "k_dl_sum", "k_dl_challenge")


def timed(call, last_ms, reps):
    """median run of `reps` calls by wall time -> (all runs sorted, the median one)"""
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        runs.append(((time.perf_counter() - t) * 1e3, last_ms()))
    runs.sort(key=lambda r: r[0])
    return runs, runs[len(runs) // 2]


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
    s = lambda: rng.randrange(1, D.R)
    secrets, recs = [], []
    for _ in range(a.distinct):                                   # random_record's drawing order
        q0, r0, q1, r1_orig, r1, z, tz = (s() for _ in range(7))
        n0, n1 = (s(), s(), s()), (s(), s(), s())
        h_q = bytes(rng.randrange(256) for _ in range(32))
        secrets.append((b"".join(D.fe(v) for v in (q0, r0, q1, r1_orig)), b"".join(D.fe(v) for v in (z, tz, r1) + n0 + n1)))
        recs.append(D.prove(key, q0, r0, q1, r1_orig, r1, z, tz, n0, n1, h_q))
    rows = D.pack([D.record_bytes(key, r) for r in recs])         # committed, com1, comz, h_q, m, pi0_c, pi0_s, pi1_c, pi1_s
    cols = [np.frombuffer(b, np.uint8).reshape(a.distinct, -1) for b in rows]
    opens = np.stack([np.frombuffer(o, np.uint8) for o, _ in secrets])
    rands = np.stack([np.frombuffer(r, np.uint8) for _, r in secrets])
    digests = np.stack([np.frombuffer(r.digest, np.uint8) for r in recs])
    res = {"layout": key.io, "h_len": 32, "distinct": a.distinct, "library": os.path.basename(cc.library_path()), "reps": a.reps, "sizes": {}}
    for n in [int(x) for x in a.sizes.split(",")]:
        idx = np.arange(n) % a.distinct
        committed, h_q = cols[0][idx].reshape(-1).copy(), cols[3][idx].reshape(-1).copy()
        openings, rand = opens[idx].reshape(-1).copy(), rands[idx].reshape(-1).copy()
        make = lambda: cc.Groth16.device_link_prove_batch_packed(pvk, key.io, key.pos0, key.pos1, committed, openings, rand, h_q, h_len=32)
        com1, comz, m, c0, s0, c1, s1, e, status = make()        # warm-up, buffer growth
        assert (status == cc.CG_SHOW_MADE).all() and np.array_equal(e, digests[idx])
        for got, j in ((com1, 1), (comz, 2), (m, 4), (c0, 5), (s0, 6), (c1, 7), (s1, 8)):
            assert np.array_equal(got.reshape(n, -1), cols[j][idx]), j
        made = [x.reshape(-1).copy() for x in (com1, comz, h_q, m, c0, s0, c1, s1)]
        verify = lambda: cc.Groth16.device_link_verify_batch_packed(pvk, key.io, key.pos0, key.pos1, committed, *made, h_len=32)
        verdicts, parts, e_v = verify()
        assert (verdicts == cc.CG_VERIFY_ACCEPT).all() and np.array_equal(e_v, e)
        runs, (wall, ms) = timed(make, pvk.device_link_prove_last_kernel_ms, a.reps)
        v_runs, (v_wall, v_ms) = timed(verify, pvk.device_link_last_kernel_ms, a.reps)
        res["sizes"][str(n)] = {"median_ms": wall, "min_ms": runs[0][0], "spread_ms": runs[-1][0] - runs[0][0], "kernel_ms": dict(zip(KERNELS, ms)),
                                "kernels_ms": sum(ms), "per_s": n / (wall / 1e3),
                                "verify": {"median_ms": v_wall, "min_ms": v_runs[0][0], "spread_ms": v_runs[-1][0] - v_runs[0][0],
                                           "kernel_ms": dict(zip(VERIFY_KERNELS, v_ms)), "kernels_ms": sum(v_ms), "per_s": n / (v_wall / 1e3)}}
    pvk.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
