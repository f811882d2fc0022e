"""Wall time of range proofs in one call each way (cg_range_prove_batch, cg_range_verify_proofs_batch: the Merlin
transcripts on the GPU) beside the multi-call entries they complete, at n_bits = 32 under a synthetic KZG key, for batches of
distinct openings.  Per size, alternating within one process, median of --reps calls after a warm-up:

  prove   one_call      cg_range_prove_batch
          multi_call    cg_range_commit_batch + cg_range_quotient_batch + cg_range_open_batch + cg_range_respond_batch fed the
                        challenges the one call derived: the multi-call path WITHOUT its host transcripts, a lower bound
          host_dleq     cg_dlog_challenge_batch for the same showings: the DLEQ transcripts on the library's host threads,
                        one of the two transcripts such a host runs per showing
  verify  one_call      cg_range_verify_proofs_batch
          multi_call    cg_range_verify_batch fed c and rho, again without its host transcripts

The multi-call outputs are compared byte for byte with the one call's before anything is timed, and every verdict is
ACCEPT.  The calls are synchronous, so what is timed is the call: copies, kernels, the stream synchronisation.  Prints one
JSON line.

    python tools/probe_range_one_call.py [--n-bits 32] [--sizes 1,256,4096,32768] [--reps 7] [--out FILE]
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


def _alternate(fns, reps):
    """{name: (median ms, min ms)} of the calls run in turn, reps rounds"""
    runs = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            t = time.perf_counter()
            fn()
            runs[name].append((time.perf_counter() - t) * 1e3)
    return {name: {"median_ms": statistics.median(v), "min_ms": min(v)} for name, v in runs.items()}


def _scalars(rng, count):
    a = rng.integers(0, 256, size=(count, 32), dtype=np.uint8)
    a[:, 31] %= 0x30
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-bits", type=int, default=32)
    ap.add_argument("--sizes", default="1,256,4096,32768")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import bn254_oracle as o
    import crescent_credentials_amd as cc
    import range_vectors as RV
    import range_verify_vectors as V
    assert cc.lib().cg_init(0, None) == 0, cc.lib().cg_last_error()
    nb = a.n_bits
    K = RV.key(nb)
    b0, b1 = 0x1234567, 0x89ABCDEF123
    pair = [o.g1_uncompressed(RV.g1(b0)), o.g1_uncompressed(RV.g1(b1))]
    pk, vk = cc.RangeProofKey(K.data, nb), cc.RangeVerifyingKey(V.vk_bytes(K), nb)
    slot, vslot = pk.add_bases(*pair), vk.add_bases(*pair)
    cfb = b"".join(o.g1_uncompressed(P) for P in K.pgam[:3] + [K.pg[0]])
    rng = np.random.default_rng(2031)
    G = cc.Groth16
    res = {"n_bits": nb, "library": os.path.basename(cc.library_path()), "reps": a.reps, "sizes": {}}
    for n in [int(s) for s in a.sizes.split(",")]:
        openings = _scalars(rng, 2 * n).reshape(n, 2, 32)
        openings[:, 0, max(nb // 8, 1):] = 0                           # m < 2^n_bits
        if nb < 8:
            openings[:, 0, 0] &= (1 << nb) - 1
        rand = _scalars(rng, 18 * n).reshape(n, 18, 32)
        # ped_com = m B_0 + r B_1 = (m b_0 + r b_1) G through the library's fixed-base entry: n pure-Python MSMs would take minutes
        val = lambda row: int.from_bytes(row.tobytes(), "little")
        logs = b"".join(((val(openings[i, 0]) * b0 + val(openings[i, 1]) * b1) % RV.R).to_bytes(32, "little") for i in range(n))
        ped = np.frombuffer(cc.fixed_base_g1(logs), np.uint8).reshape(n, 64).copy()
        one = lambda: G.range_prove_batch_packed(pk, slot, openings, ped, rand)
        com_f, com_g, com_q, evals, proofs, pok_c, pok_s, chal, status = one()
        assert (status == cc.CG_SHOW_MADE).all()
        c_dleq, c, rho = (np.ascontiguousarray(chal[:, j]) for j in range(3))
        ts = [None]

        def multi():
            f, g, t, _ = G.range_commit_batch_packed(pk, slot, openings, rand)
            q, _, _ = G.range_quotient_batch_packed(pk, openings, rand, c)
            e, p, st = G.range_open_batch_packed(pk, openings, rand, c, rho)
            s = G.range_respond_batch(openings, rand, c_dleq, st)
            ts[0] = t
            return f, g, q, e, p, s

        for mine, theirs in zip(multi(), (com_f, com_g, com_q, evals, proofs, pok_s)):
            assert mine.tobytes() == theirs.tobytes()
        k = np.ascontiguousarray(ts[0][:, 2:])
        host_dleq = lambda: G.dlog_challenge_batch([2, 4], b"".join(pair) + cfb, k, ped, com_f)
        assert host_dleq().tobytes() == pok_c.tobytes()
        rz = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        v_one = lambda: G.range_verify_proofs_batch_packed(vk, vslot, ped, com_f, com_g, com_q, evals, proofs, rz, pok_c, pok_s)
        v_multi = lambda: G.range_verify_batch_packed(vk, vslot, ped, com_f, com_g, com_q, evals, proofs, c, rho, rz, pok_c, pok_s)
        assert (v_one() == cc.CG_VERIFY_ACCEPT).all() and (v_multi()[0] == cc.CG_VERIFY_ACCEPT).all()
        t = {"prove": _alternate({"one_call": one, "multi_call": multi, "host_dleq": host_dleq}, a.reps),
             "verify": _alternate({"one_call": v_one, "multi_call": v_multi}, a.reps)}
        for side in t.values():
            for v in side.values():
                v["per_s"] = n / (v["median_ms"] / 1e3)
        res["sizes"][str(n)] = t
    pk.close()
    vk.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
