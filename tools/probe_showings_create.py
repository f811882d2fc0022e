"""Wall time of creating whole showings in one call (cg_create_showings_batch) beside the sequence of separate calls it
replaces, under a synthetic gamma = 1 key with 26 public inputs in the JWT-like layout of profiles/showing_verify.md
(2 committed, 6 hidden, 18 revealed) and one 32-bit range proof on the first committed input; one client state duplicated n
times, every showing with the same random scalars (the arithmetic does not depend on them).  Per size, alternating within one
process, median of --reps calls after a warm-up:

  whole_overlap     cg_create_showings_batch, the range half started beside k_mk_var (cg_pvk_set_showings_overlap 1)
  whole_in_turn     the same call with the range half started behind the Groth16 half (0)
  separate          cg_show_commit_batch, cg_dlog_challenge_batch on the host, cg_show_respond_batch on the host,
                    cg_show_shift_batch and cg_range_prove_batch, each fed what the one before brought down

Every output array of the three variants is byte-equal, and every showing made, before anything is timed.  `spread_ms` is
max - min of a variant's runs: the yardstick for "not slower than".  The calls are synchronous, so what is timed is the call:
copies, kernels, the stream synchronisation.  Prints one JSON line.

    python tools/probe_showings_create.py [--sizes 1,1024,16384] [--reps 7] [--out FILE]
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
    runs = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            t = time.perf_counter()
            fn()
            runs[name].append((time.perf_counter() - t) * 1e3)
    return {name: {"median_ms": statistics.median(v), "min_ms": min(v), "spread_ms": max(v) - min(v)} for name, v in runs.items()}


def _flat(res):
    """every array of a result, in one fixed order, as bytes"""
    rp, comh, comm, c, s, ranges, status, parts = res
    return [a.tobytes() for a in (rp, comh, comm, c, s, status, parts)] + [a.tobytes() for r in ranges for a in r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,1024,16384")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import bn254_oracle as o
    import crescent_credentials_amd as cc
    import range_vectors as RV
    import show_vectors as S
    import verify_vectors as V
    assert cc.lib().cg_init(0, None) == 0, cc.lib().cg_last_error()
    G, R = cc.Groth16, o.R
    ell, n_bits, context = 26, 32, b"presentation message"
    io = S.jwt_like_layout(ell)
    com = [i for i, t in enumerate(io) if t == S.COMMITTED]
    hid = [i for i, t in enumerate(io) if t == S.HIDDEN]
    rng, sc = V.synthetic_scalars(ell, 0x5A0E, gamma=1)
    vk = V.synthetic_vk(*sc[:4], sc[4])
    pvk = cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(vk)))
    K = RV.key(n_bits)
    rpk = cc.RangeProofKey(K.data, n_bits)
    pos = com[0]
    slot = rpk.add_bases(o.g1_uncompressed(vk["gamma_abc_g1"][pos + 1]), o.g1_uncompressed(vk["delta_g1"]))
    # one client state: the first committed input = cur_time + a 32-bit value
    t = 1_800_000_000
    xs = [rng.randrange(R) for _ in range(ell)]
    xs[pos] = t + rng.randrange(1 << n_bits)
    n_rand = cc.show_rand_count(io)
    fe = lambda v: int(v).to_bytes(32, "little")
    one = dict(proofs=V.proof_bytes(V.synthetic_proof(sc, xs, a=rng.randrange(1, R), b=rng.randrange(1, R))), inputs=b"".join(fe(x) for x in xs),
               rand=b"".join(fe(rng.randrange(1, R)) for _ in range(n_rand)), shifts=fe(t),
               range_rand=b"".join(fe(rng.randrange(R)) for _ in range(cc.CG_RANGE_N_RAND)))
    abc, delta = pvk.gamma_abc_g1, pvk.delta_g1
    bases = np.concatenate([x for i in com for x in (abc[i + 1], delta)] + [abc[j + 1] for j in hid] + [delta])
    n_bases = [2] * len(com) + [len(hid) + 1]
    res = {"ell": ell, "n_bits": n_bits, "library": os.path.basename(cc.library_path()), "reps": a.reps, "sizes": {}}
    for n in [int(s) for s in a.sizes.split(",")]:
        r = {k: np.tile(np.frombuffer(bytes(v), np.uint8), (n, 1)) for k, v in one.items()}

        def whole():
            return G.create_showings_batch_packed(pvk, rpk, io, r["proofs"], r["inputs"], r["rand"], [(0, slot)], r["shifts"], r["range_rand"], context)

        def separate():
            rp, comh, comm, k, status = G.show_commit_batch_packed(pvk, io, r["proofs"], r["inputs"], r["rand"])
            c = G.dlog_challenge_batch(n_bases, bases, k, comm, comh, context)
            s = G.show_respond_batch(io, r["inputs"], r["rand"], c, status)
            # the opening the host assembles itself: m = inputs[pos], r = the r_i it drew
            openings = np.concatenate([r["inputs"].reshape(n, ell, 32)[:, pos], r["rand"].reshape(n, n_rand, 32)[:, 2]], axis=1)
            out, ped, st = G.show_shift_batch(pvk, pos, openings, comm[:, 0].copy(), r["shifts"])
            made = G.range_prove_batch_packed(rpk, slot, out, ped, r["range_rand"])
            parts = np.stack([status, np.where((st == cc.CG_SHOW_MADE) & (made[8] == cc.CG_SHOW_MADE), cc.CG_SHOW_MADE, cc.CG_SHOW_MALFORMED)], axis=1)
            return rp, comh, comm, c, s, [made[:8]], status, parts.astype(np.uint8)

        def in_turn():
            pvk.set_showings_overlap(False)
            try:
                return whole()
            finally:
                pvk.set_showings_overlap(True)

        first = whole()
        assert (first[6] == cc.CG_SHOW_MADE).all() and (first[7] == cc.CG_SHOW_MADE).all()
        assert _flat(first) == _flat(separate()) and _flat(first) == _flat(in_turn())
        times = _alternate({"whole_overlap": whole, "whole_in_turn": in_turn, "separate": separate}, a.reps)
        for v in times.values():
            v["per_s"] = n / (v["median_ms"] / 1e3)
        res["sizes"][str(n)] = times
    for h in (pvk, rpk):
        h.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
