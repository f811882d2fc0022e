"""What h_Q on the GPU costs (cg_hq_batch, cg_device_link_prove_hq_batch, csrc/devicelinkmake.hip), under the key, the layout and
the scalars of tools/probe_device_link_create.py: the mDL-like layout [COMMITTED, HIDDEN, COMMITTED, COMMITTED, REVEALED] with
the device keys at inputs 2 and 3, 64 distinct proofs repeated to the batch size.  h_Q of each proof is tests/poseidon_vectors.py's,
and before anything is timed every output row of both proving calls must be the pure-Python prover's fed that h_Q, and
cg_hq_batch's rows must be Python's.  Per size, in ONE run:

    parent      cg_device_link_prove_batch with h_Q supplied: median wall ms of --reps calls, three times over (the run-to-run
                spread of the figure the new call is held against)
    with_hq     cg_device_link_prove_hq_batch: median wall ms, and of the run with the median wall time the HIP-event time of
                k_hq_link (cg_hq_last_kernel_ms) and of the six kernels behind it
    hq_alone    cg_hq_batch: median wall ms and its kernel's event time
    host        one thread of the g++ build of csrc/poseidon_p256.hpp (tests/cpp/test_poseidon_p256.cpp, `time`): ns per hash
                over --host-hashes hashes, times n

and the condition with_hq <= parent + host / 16 (a host with 16 threads and no other work).  Prints one JSON line.

    python tools/probe_device_link_hq.py [--sizes 1,1024,16384] [--reps 7] [--distinct 64] [--host-hashes 512] [--out FILE]
"""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

KERNELS = ("k_dlm_check", "k_dlm_terms", "k_dlm_sum", "k_dlm_pi0", "k_dlm_lhs1", "k_dlm_pi1")


def timed(call, last_ms, reps):
    """median run of `reps` calls by wall time -> (all runs sorted, the median one)"""
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        runs.append(((time.perf_counter() - t) * 1e3, last_ms()))
    runs.sort(key=lambda r: r[0])
    return runs, runs[len(runs) // 2]


def host_ns_per_hash(hashes):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "test_poseidon_p256")
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_poseidon_p256.cpp")], check=True,
                       capture_output=True)
        r = subprocess.run([exe], input="time %d\n" % hashes, capture_output=True, text=True, check=True)
        return float(r.stdout.split()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,1024,16384")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--host-hashes", type=int, default=512)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import crescent_credentials_amd as cc
    import device_link_vectors as D
    import poseidon_vectors as PV
    import verify_vectors as V
    assert cc.lib().cg_init(0, None) == 0, cc.lib().cg_last_error()
    key = D.make_key([D.COMMITTED, D.HIDDEN, D.COMMITTED, D.COMMITTED, D.REVEALED], 2, 3, 0xDE71CE)
    pvk = cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(key.vk)))
    rng = random.Random(0x9B0BE)
    s = lambda: rng.randrange(1, D.R)
    secrets, recs, triples = [], [], []
    for _ in range(a.distinct):
        q0, r0, q1, r1_orig, r1, z, tz = (s() for _ in range(7))
        n0, n1 = (s(), s(), s()), (s(), s(), s())
        secrets.append((b"".join(D.fe(v) for v in (q0, r0, q1, r1_orig)), b"".join(D.fe(v) for v in (z, tz, r1) + n0 + n1)))
        triples.append(b"".join(D.fe(v) for v in (q0, q1, z)))
        recs.append(D.prove(key, q0, r0, q1, r1_orig, r1, z, tz, n0, n1, PV.hq(q0, q1, z)))
    rows = D.pack([D.record_bytes(key, r) for r in recs])         # committed, com1, comz, h_q, m, pi0_c, pi0_s, pi1_c, pi1_s
    cols = [np.frombuffer(b, np.uint8).reshape(a.distinct, -1) for b in rows]
    opens = np.stack([np.frombuffer(o, np.uint8) for o, _ in secrets])
    rands = np.stack([np.frombuffer(r, np.uint8) for _, r in secrets])
    qs = np.stack([np.frombuffer(t, np.uint8) for t in triples])
    digests = np.stack([np.frombuffer(r.digest, np.uint8) for r in recs])
    host_ns = host_ns_per_hash(a.host_hashes)
    res = {"layout": key.io, "distinct": a.distinct, "library": os.path.basename(cc.library_path()), "reps": a.reps, "host_ns_per_hash": host_ns,
           "host_hashes_timed": a.host_hashes, "sizes": {}}
    G = cc.Groth16
    for n in [int(x) for x in a.sizes.split(",")]:
        idx = np.arange(n) % a.distinct
        committed, h_q, q = cols[0][idx].reshape(-1).copy(), cols[3][idx].reshape(-1).copy(), qs[idx].reshape(-1).copy()
        openings, rand = opens[idx].reshape(-1).copy(), rands[idx].reshape(-1).copy()
        parent = lambda: G.device_link_prove_batch_packed(pvk, key.io, key.pos0, key.pos1, committed, openings, rand, h_q, h_len=32)
        with_hq = lambda: G.device_link_prove_hq_batch_packed(pvk, key.io, key.pos0, key.pos1, committed, openings, rand)
        alone = lambda: G.hq_batch_packed(pvk, q)
        for out in (parent(), with_hq()):                          # warm-up, buffer growth, and the bytes
            com1, comz, m, c0, s0, c1, s1, e, status = out[:9]
            assert (status == cc.CG_SHOW_MADE).all() and np.array_equal(e, digests[idx])
            for got, j in ((com1, 1), (comz, 2), (m, 4), (c0, 5), (s0, 6), (c1, 7), (s1, 8)):
                assert np.array_equal(got.reshape(n, -1), cols[j][idx]), j
            assert len(out) == 9 or np.array_equal(out[9], cols[3][idx])
        h, h_status = alone()
        assert (h_status == cc.CG_SHOW_MADE).all() and np.array_equal(h, cols[3][idx])
        parents = [timed(parent, pvk.device_link_prove_last_kernel_ms, a.reps) for _ in range(3)]
        runs, (wall, (ms_link, ms)) = timed(with_hq, lambda: (pvk.hq_last_kernel_ms()[1], pvk.device_link_prove_last_kernel_ms()), a.reps)
        a_runs, (a_wall, a_ms) = timed(alone, lambda: pvk.hq_last_kernel_ms()[0], a.reps)
        p_medians = [med[0] for _, med in parents]
        p_wall = sorted(p_medians)[1]
        host_ms = host_ns * n / 1e6
        res["sizes"][str(n)] = {
            "parent": {"median_ms": p_wall, "medians_ms": p_medians, "run_to_run_spread_ms": max(p_medians) - min(p_medians),
                       "kernel_ms": dict(zip(KERNELS, parents[1][1][1]))},
            "with_hq": {"median_ms": wall, "min_ms": runs[0][0], "spread_ms": runs[-1][0] - runs[0][0], "k_hq_link_ms": ms_link,
                        "kernel_ms": dict(zip(KERNELS, ms)), "per_s": n / (wall / 1e3)},
            "hq_alone": {"median_ms": a_wall, "min_ms": a_runs[0][0], "spread_ms": a_runs[-1][0] - a_runs[0][0], "k_hq_hash_ms": a_ms,
                         "per_s": n / (a_wall / 1e3)},
            "host_one_thread_ms": host_ms,
            "condition": {"with_hq_ms": wall, "parent_plus_sixteenth_of_host_ms": p_wall + host_ms / 16, "holds": wall <= p_wall + host_ms / 16}}
    pvk.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
