"""Wall time of cg_verify_show_batch (showings on the GPU, csrc/verify.hip) at a synthetic gamma = 1 key with ell public
inputs and the JWT-like layout (two committed inputs, several hidden, the rest revealed) for several batch sizes: one valid
showing duplicated n times, verdicts and k bytes checked against the oracle.  cg_verify_batch runs on the same key and n
in the same process as the comparison (the show call does strictly more work).  Prints one JSON line; run it under
`rocprofv3 --kernel-trace --stats -- python tools/probe_verify_show.py --reps 2` for the per-kernel times.

    python tools/probe_verify_show.py [--ell 26] [--sizes 1,64,1024,16384] [--reps 5] [--out FILE]
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
    ap.add_argument("--sizes", default="1,64,1024,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import crescent_credentials_amd as cc
    import bn254_oracle as o
    import show_vectors as S
    import verify_vectors as V
    assert cc.lib().cg_init(0, None) == 0, cc.lib().cg_last_error()
    rng = random.Random(2026)
    R = V.R
    alpha, beta, delta = (rng.randrange(1, R) for _ in range(3))
    sc = (alpha, beta, 1, delta, [rng.randrange(R) for _ in range(a.ell + 1)])
    xs = [rng.randrange(R) for _ in range(a.ell)]
    vk = V.synthetic_vk(*sc[:4], sc[4])
    proof = V.synthetic_proof(sc, xs, a=rng.randrange(1, R), b=rng.randrange(1, R))
    io = S.jwt_like_layout(a.ell)
    sh = S.make_show(vk, proof, xs, io, rng)
    want_k = np.frombuffer(S.k_bytes(sh.k), np.uint8)
    t0 = time.perf_counter()
    pvk_bytes = cc.Groth16.prepare_verifying_key(V.vk_bytes(vk))
    t1 = time.perf_counter()
    pvk = cc.PreparedVerifyingKey(pvk_bytes)
    t2 = time.perf_counter()
    res = {"ell": a.ell, "n_revealed": io.count(S.REVEALED), "n_hidden": io.count(S.HIDDEN), "n_committed": io.count(S.COMMITTED),
           "prepare_verifying_key_ms": (t1 - t0) * 1e3, "pvk_load_ms": (t2 - t1) * 1e3, "sizes": {}}
    fe = lambda vals: np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in vals), np.uint8)
    one = dict(revealed=fe(sh.revealed), rand_proofs=np.frombuffer(o.proof_uncompressed(sh.rand_proof), np.uint8),
               com_hidden=np.frombuffer(o.g1_uncompressed(sh.com_hidden), np.uint8),
               committed=np.frombuffer(b"".join(o.g1_uncompressed(P) for P in sh.committed), np.uint8),
               pok_c=fe([sh.c]), pok_s=fe([x for si in sh.s for x in si]))
    plain_in, plain_pr = fe(xs), np.frombuffer(V.proof_bytes(proof), np.uint8)
    for n in [int(s) for s in a.sizes.split(",")]:
        args = {k: np.tile(v, n) for k, v in one.items()}
        v, k = cc.Groth16.verify_show_batch_packed(pvk, io, **args)          # warm-up (and buffer growth)
        assert (v == cc.CG_VERIFY_ACCEPT).all() and (k.reshape(n, -1) == want_k).all()
        half = dict(args, pok_c=None, pok_s=None)
        ib, pb = np.tile(plain_in, n), np.tile(plain_pr, n)
        assert (cc.Groth16.verify_batch(pvk, ib, pb) == cc.CG_VERIFY_ACCEPT).all()
        show_ms, show_min = _median_ms(lambda: cc.Groth16.verify_show_batch_packed(pvk, io, **args), a.reps)
        half_ms, _ = _median_ms(lambda: cc.Groth16.verify_show_batch_packed(pvk, io, **half), a.reps)
        plain_ms, _ = _median_ms(lambda: cc.Groth16.verify_batch(pvk, ib, pb), a.reps)
        res["sizes"][str(n)] = {"show_median_ms": show_ms, "show_min_ms": show_min, "showings_per_s": n / (show_ms / 1e3),
                                "groth16_half_only_median_ms": half_ms, "verify_batch_median_ms": plain_ms,
                                "show_over_verify_batch": show_ms / plain_ms}
    pvk.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
