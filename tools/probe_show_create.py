"""Wall time of cg_show_commit_batch (creating showings on the GPU, csrc/verify.hip) at a synthetic gamma = 1 key with ell
public inputs and the JWT-like layout (two committed inputs, several hidden, the rest revealed): one client state under
one set of random values duplicated n times, every output byte of every row checked against the oracle's showing.  The
call is synchronous and works on the handle's own stream, so what is timed is the call itself: both copies, four kernels
and the stream synchronisation.  cg_show_respond_batch (host) and cg_verify_show_batch on the showings just made run in the
same process as the comparison.  Prints one JSON line; run it under
`rocprofv3 --kernel-trace --stats -- python tools/probe_show_create.py --reps 2` for the per-kernel times.

    python tools/probe_show_create.py [--ell 26] [--sizes 32768] [--reps 5] [--out FILE]
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


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts) * 1e3, min(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ell", type=int, default=26)
    ap.add_argument("--sizes", default="32768")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import crescent_credentials_amd as cc
    import show_create_vectors as M
    import show_vectors as S
    import verify_vectors as V
    assert cc.lib().cg_init(0, None) == 0, cc.lib().cg_last_error()
    rng, sc, vk, xs, abc = M.synthetic(a.ell, 2027)
    io = S.jwt_like_layout(a.ell)
    n_com, n_hid, n_resp, n_rand = M.counts(io)
    m = M.make(vk, M.proof_of(abc), xs, io, rng)
    want = [np.frombuffer(w, np.uint8) for w in M.expected(io, m)]
    t0 = time.perf_counter()
    pvk = cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(vk)))
    res = {"ell": a.ell, "n_revealed": io.count(S.REVEALED), "n_hidden": n_hid, "n_committed": n_com, "n_rand": n_rand,
           "fixed_base_terms": 2 * n_resp + 1, "prepare_and_pvk_load_ms": (time.perf_counter() - t0) * 1e3, "sizes": {}}
    proofs1, inputs1, rand1 = (x.reshape(-1) for x in M.pack([m]))
    for n in [int(s) for s in a.sizes.split(",")]:
        proofs, inputs, rand = np.tile(proofs1, n), np.tile(inputs1, n), np.tile(rand1, n)
        rp, comh, comm, k, status = cc.Groth16.show_commit_batch_packed(pvk, io, proofs, inputs, rand)     # warm-up, buffer growth
        assert (status == cc.CG_SHOW_MADE).all()
        for got, w in zip((rp, comh, comm, k), want):
            assert (got.reshape(n, -1) == w).all()
        c = np.tile(np.frombuffer(int(m.show.c).to_bytes(32, "little"), np.uint8), n)
        s = cc.Groth16.show_respond_batch(io, inputs, rand, c, status)
        assert (s.reshape(n, -1) == want[4]).all()
        revealed = np.tile(np.frombuffer(M.fe(m.show.revealed), np.uint8), n)
        verify = lambda: cc.Groth16.verify_show_batch_packed(pvk, io, revealed, rp, comh, comm, c, s)
        v, k2 = verify()
        assert (v == cc.CG_VERIFY_ACCEPT).all() and (k2 == k).all()
        commit_ms, commit_min = _median_ms(lambda: cc.Groth16.show_commit_batch_packed(pvk, io, proofs, inputs, rand), a.reps)
        respond_ms, _ = _median_ms(lambda: cc.Groth16.show_respond_batch(io, inputs, rand, c, status), a.reps)
        verify_ms, verify_min = _median_ms(verify, a.reps)
        res["sizes"][str(n)] = {"commit_median_ms": commit_ms, "commit_min_ms": commit_min, "showings_per_s": n / (commit_ms / 1e3),
                                "respond_host_median_ms": respond_ms, "verify_show_median_ms": verify_ms, "verify_show_min_ms": verify_min,
                                "commit_over_verify_show": commit_ms / verify_ms}
    pvk.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
