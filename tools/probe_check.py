"""What the witness check costs (cg_check_witness, CG_FLAG_CHECK_WITNESS; csrc/wmap29.hip k_sat_check29) at a synthetic
circuit of the bench's shape: `check_ms` of cg_check_witness alone, and proofs/s and lone-proof latency of a 16-slot
throughput context loaded WITHOUT and WITH the flag, measured in alternation (profiles/witness_check.md).  Prints one
JSON line; run it under `rocprofv3 --kernel-trace --stats -- python tools/probe_check.py --rounds 1` for the per-kernel times.

    python tools/probe_check.py [--shape rs256] [--slots 16] [--proofs 160] [--rounds 3] [--lone 20] [--out FILE]
"""
import argparse
import json
import os
import random
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def _rate(prover, hb_ptr, n_threads, n_proofs, want):
    """n_proofs proofs from n_threads threads -> proofs/s; every proof compared with `want`"""
    per = n_proofs // n_threads
    bad = []
    start = threading.Barrier(n_threads + 1)

    def run():
        start.wait()
        for _ in range(per):
            if prover.prove_host_ptr(hb_ptr, 3, 4).data != want:
                bad.append(1)

    ts = [threading.Thread(target=run) for _ in range(n_threads)]
    for t in ts:
        t.start()
    start.wait()
    t0 = time.perf_counter()
    for t in ts:
        t.join()
    dt = time.perf_counter() - t0
    assert not bad, "proof bytes differ"
    return per * n_threads / dt


def _lone_ms(prover, hb_ptr, n):
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        prover.prove_host_ptr(hb_ptr, 3, 4)
        ts.append((time.perf_counter() - t) * 1e3)
        time.sleep(0.02)                                   # a server between requests: the context is empty again
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="rs256")
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--proofs", type=int, default=160, help="proofs per rate measurement")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds (unflagged, flagged)")
    ap.add_argument("--lone", type=int, default=20, help="lone proofs per latency measurement")
    ap.add_argument("--checks", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import crescent_credentials_amd as cc
    from crescent_credentials_amd import workloads as wl
    assert cc.lib().cg_init(0, None) == 0, cc.lib().cg_last_error()
    l, m, M = wl.SHAPES[a.shape]
    cm, w = wl.synthetic_circuit(0xC5E5CE47, l, m, M, 0.9, 3, profile="gates")
    rng = random.Random(7)
    pk = cc.generate_parameters_with_qap(cm, *[rng.randrange(1, R) for _ in range(4)])
    hb = cc.HostBuffer(M * 32)
    hb.array[:] = w
    res = {"shape": a.shape, "l": l, "m": m, "M": M, "slots": a.slots, "proofs_per_measurement": a.proofs, "rounds": []}
    provers = {}
    for name, flag in (("unflagged", False), ("flagged", True)):
        provers[name] = cc.Prover(pk, cm, proof_slots=a.slots, check_witness=flag)
    try:
        want = provers["unflagged"].prove_host_ptr(hb.ptr, 3, 4).data
        assert provers["flagged"].prove_host_ptr(hb.ptr, 3, 4).data == want
        for p in provers.values():                          # warm-up: the one-time window re-tune and the clocks
            _rate(p, hb.ptr, a.slots, 2 * a.slots, want)
        # cg_check_witness alone, on the idle unflagged context
        cms = []
        for _ in range(a.checks):
            rep = provers["unflagged"].check_witness(w)
            assert rep.satisfied
            cms.append(rep.check_ms)
        res["check_ms"] = {"median": statistics.median(cms), "min": min(cms), "max": max(cms), "n": len(cms)}
        w_bad = w.copy()
        w_bad[32 * (M - 1)] ^= 1
        rep = provers["unflagged"].check_witness(w_bad)
        res["check_ms_unsatisfied"] = {"n_unsatisfied": rep.n_unsatisfied, "check_ms": rep.check_ms}
        for rd in range(a.rounds):
            row = {}
            for name in ("unflagged", "flagged"):
                row[name] = {"proofs_per_s": round(_rate(provers[name], hb.ptr, a.slots, a.proofs, want), 2),
                             "lone_proof_ms": round(_lone_ms(provers[name], hb.ptr, a.lone), 3)}
            res["rounds"].append(row)
        for name in ("unflagged", "flagged"):
            res[name + "_proofs_per_s"] = [r_[name]["proofs_per_s"] for r_ in res["rounds"]]
            res[name + "_lone_proof_ms"] = [r_[name]["lone_proof_ms"] for r_ in res["rounds"]]
    finally:
        for p in provers.values():
            p.close()
        hb.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
