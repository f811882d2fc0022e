"""Wall time of verifying whole showings in one call (cg_verify_showings_batch) beside the sequence of separate calls it
replaces, under a synthetic gamma = 1 key with 26 public inputs in the JWT-like layout of profiles/verify_show_batch_ell26.md
(2 committed, 6 hidden, 18 revealed) and one 32-bit range proof on the first committed input; one valid showing made by the
library (show_batch, show_shift_batch, prove_range_batch) and duplicated n times.  Per size, alternating within one process,
median of --reps calls after a warm-up:

  whole_overlap     cg_verify_showings_batch, the range half started beside the Groth16 half (cg_pvk_set_showings_overlap 1)
  whole_in_turn     the same call with the range half started behind the Groth16 half (0)
  separate          cg_verify_show_batch, then cg_dlog_challenge_batch on the host, then cg_range_verify_proofs_batch with a
                    ped_com prepared beforehand and not timed: the separate calls cannot compute it

Every verdict is ACCEPT and the part verdicts equal the separate calls' before anything is timed.  `spread_ms` is max - min of
a variant's runs: the yardstick for "not slower than".  With --latency both handles are in latency mode.  The calls are
synchronous, so what is timed is the call: copies, kernels, the stream synchronisation.  Prints one JSON line.

    python tools/probe_showings_whole.py [--sizes 1,1024,16384] [--reps 7] [--latency] [--out FILE]
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


def _alternate(fns, reps):
    runs = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            t = time.perf_counter()
            fn()
            runs[name].append((time.perf_counter() - t) * 1e3)
    return {name: {"median_ms": statistics.median(v), "min_ms": min(v), "spread_ms": max(v) - min(v)} for name, v in runs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,1024,16384")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--latency", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import bn254_oracle as o
    import crescent_credentials_amd as cc
    import range_vectors as RV
    import range_verify_vectors as RVV
    import show_vectors as S
    import verify_vectors as V
    assert cc.lib().cg_init(0, None) == 0, cc.lib().cg_last_error()
    G, R = cc.Groth16, o.R
    ell, n_bits, context = 26, 32, b"presentation message"
    io = S.jwt_like_layout(ell)
    rng, sc = V.synthetic_scalars(ell, 0x5A0E, gamma=1)
    vk = V.synthetic_vk(*sc[:4], sc[4])
    pvk = cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(vk)), latency=a.latency)
    K = RV.key(n_bits)
    rpk, rvk = cc.RangeProofKey(K.data, n_bits), cc.RangeVerifyingKey(RVV.vk_bytes(K), n_bits, latency=a.latency)
    pair = [o.g1_uncompressed(vk["gamma_abc_g1"][1]), o.g1_uncompressed(vk["delta_g1"])]
    pslot, vslot = rpk.add_bases(*pair), rvk.add_bases(*pair)
    # one showing: input 0 = cur_time + a 32-bit value
    t = 1_800_000_000
    xs = [rng.randrange(R) for _ in range(ell)]
    xs[0] = t + rng.randrange(1 << n_bits)
    row = [rng.randrange(1, R) for _ in range(cc.show_rand_count(io))]
    proof = V.proof_bytes(V.synthetic_proof(sc, xs, a=rng.randrange(1, R), b=rng.randrange(1, R)))
    sg = G.show_batch(pvk, io, [(proof, xs)], rand=[row], context=context)[0]
    out, ped, status = G.show_shift_batch(pvk, 0, [(xs[0], row[2])], [sg.commited_inputs[0]], [t])
    assert status.tolist() == [cc.CG_SHOW_MADE]
    val = lambda b: int.from_bytes(b.tobytes(), "little")
    rp = G.prove_range_batch(rpk, pslot, [(val(out[0, 0]), val(out[0, 1]))], [ped[0].tobytes()])[0]
    fe = lambda v: int(v).to_bytes(32, "little")
    one = dict(revealed=b"".join(fe(x) for x, ty in zip(xs, io) if ty == S.REVEALED), rand_proofs=sg.rand_proof, com_hidden=sg.com_hidden_inputs,
               committed=b"".join(sg.commited_inputs), pok_c=fe(sg.pok_c), pok_s=b"".join(fe(s) for si in sg.pok_s for s in si), shifts=fe(t),
               ped=ped[0].tobytes(), com_f=rp.com_f, com_g=rp.com_g, com_q=rp.com_q, evals=fe(rp.eval_g) + fe(rp.eval_gw) + fe(rp.eval_w_hat),
               proofs=bytes(rp.proof_g) + bytes(rp.proof_gw) + bytes(rp.proof_w_hat), rz=random.Random(5).getrandbits(256).to_bytes(32, "little"),
               rpok_c=fe(rp.dleq_c), rpok_s=b"".join(fe(s) for si in rp.dleq_s for s in si))
    res = {"ell": ell, "n_bits": n_bits, "latency": bool(a.latency), "library": os.path.basename(cc.library_path()), "reps": a.reps, "sizes": {}}
    for n in [int(s) for s in a.sizes.split(",")]:
        r = {k: np.tile(np.frombuffer(bytes(v), np.uint8), (n, 1)) for k, v in one.items()}
        ranges = [(r["com_f"], r["com_g"], r["com_q"], r["evals"], r["proofs"], r["rz"], r["rpok_c"], r["rpok_s"])]

        def whole():
            return G.verify_showings_batch_packed(pvk, rvk, io, r["revealed"], r["rand_proofs"], r["com_hidden"], r["committed"], r["pok_c"],
                                                  r["pok_s"], [(0, vslot)], r["shifts"], ranges, context)

        def separate():
            verdicts, k = G.verify_show_batch_packed(pvk, io, r["revealed"], r["rand_proofs"], r["com_hidden"], r["committed"], r["pok_c"], r["pok_s"])
            cs = G.show_dlog_challenges(pvk, io, k, r["committed"], r["com_hidden"], context)
            rv = G.range_verify_proofs_batch_packed(rvk, vslot, r["ped"], r["com_f"], r["com_g"], r["com_q"], r["evals"], r["proofs"], r["rz"],
                                                    r["rpok_c"], r["rpok_s"])
            return verdicts, cs, rv

        def in_turn():
            pvk.set_showings_overlap(False)
            try:
                return whole()
            finally:
                pvk.set_showings_overlap(True)

        verdicts, parts = whole()
        sv, cs, rv = separate()
        assert (verdicts == cc.CG_VERIFY_ACCEPT).all() and (parts == cc.CG_VERIFY_ACCEPT).all()
        assert (sv == cc.CG_VERIFY_ACCEPT).all() and (rv == cc.CG_VERIFY_ACCEPT).all() and cs.tobytes() == r["pok_c"].tobytes()
        assert in_turn()[1].tobytes() == parts.tobytes()
        times = _alternate({"whole_overlap": whole, "whole_in_turn": in_turn, "separate": separate}, a.reps)
        for v in times.values():
            v["per_s"] = n / (v["median_ms"] / 1e3)
        res["sizes"][str(n)] = times
    for h in (pvk, rpk, rvk):
        h.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
