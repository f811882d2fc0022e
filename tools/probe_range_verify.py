"""Wall time of verifying range proofs on the GPU (csrc/rangeverify.hip) at n_bits = 32 under a synthetic KZG key: the load
(two G2 points prepared on the host, tables of six bases and their upload), cg_range_vk_add_bases, and
cg_range_verify_batch with a DLEQ for batches of DISTINCT proofs, which the creation calls of csrc/rangeproof.hip make on
the same GPU from distinct openings, random values and challenges (a duplicated row would walk the same table entries and
take the same branches in every lane).  Every verdict must be CG_VERIFY_ACCEPT, and row 0 - the only one whose ped_com is
the true commitment, the others carry their com_g as a stand-in curve point, which k_0 alone sees - is checked against
the trapdoor restatement of tests/range_verify_vectors.py.  The call is synchronous and works on the handle's own stream,
so what is timed is the call itself: the copies, five kernels per chunk and the stream synchronisation; next to it the
HIP-event time of the group stage and of the pairing (cg_range_vk_last_kernel_ms).  In the same run, as the yardstick,
cg_verify_batch on the same machine (the existing Groth16 verifier, one valid proof with `--ell` inputs duplicated, as
tools/probe_verify.py times it).  Prints one JSON line.

    python tools/probe_range_verify.py [--n-bits 32] [--sizes 1,256,4096,32768] [--reps 5] [--ell 26] [--out FILE]
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


def _scalars(rng, count):
    """count canonical scalars: 32 random bytes with the top one below 0x30, the scalar modulus's"""
    a = rng.integers(0, 256, size=(count, 32), dtype=np.uint8)
    a[:, 31] %= 0x30
    return a


def _groth16_yardstick(cc, ell, sizes, reps):
    import verify_vectors as VV
    rng = random.Random(2026)
    R = VV.R
    sc = tuple(rng.randrange(1, R) for _ in range(4)) + ([rng.randrange(R) for _ in range(ell + 1)],)
    xs = [rng.randrange(R) for _ in range(ell)]
    proof = VV.proof_bytes(VV.synthetic_proof(sc, xs, a=rng.randrange(1, R), b=rng.randrange(1, R)))
    pvk = cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(VV.vk_bytes(VV.synthetic_vk(*sc[:4], sc[4]))))
    ib1, pb1 = np.frombuffer(VV.inputs_bytes(xs), np.uint8), np.frombuffer(proof, np.uint8)
    out = {}
    for n in sizes:
        ib, pb = np.tile(ib1, n), np.tile(pb1, n)
        assert (cc.Groth16.verify_batch(pvk, ib, pb) == cc.CG_VERIFY_ACCEPT).all()          # warm-up, buffer growth
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            cc.Groth16.verify_batch(pvk, ib, pb)
            ts.append((time.perf_counter() - t) * 1e3)
        med = statistics.median(ts)
        out[str(n)] = {"median_ms": med, "min_ms": min(ts), "ms_per_proof": med / n, "proofs_per_s": n / (med / 1e3)}
    pvk.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latency", action="store_true", help="also time both arrangements of the pairing stage, alternated")
    ap.add_argument("--no-groth16", action="store_true", help="leave the cg_verify_batch yardstick out")
    ap.add_argument("--n-bits", type=int, default=32)
    ap.add_argument("--sizes", default="1,256,4096,32768")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ell", type=int, default=26)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import bn254_oracle as o
    import crescent_credentials_amd as cc
    import range_vectors as RV
    import range_verify_vectors as V
    assert cc.lib().cg_init(0, None) == 0, cc.lib().cg_last_error()
    nb = a.n_bits
    sizes = [int(s) for s in a.sizes.split(",")]
    K = RV.key(nb)
    bases = V.bases_of()
    base_bytes = [o.g1_uncompressed(P) for P in bases]
    pk = cc.RangeProofKey(K.data, nb)
    pk_slot = pk.add_bases(*base_bytes)
    t0 = time.perf_counter()
    vk = cc.RangeVerifyingKey(V.vk_bytes(K), nb)
    load_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    slot = vk.add_bases(*base_bytes)
    res = {"n_bits": nb, "library": os.path.basename(cc.library_path()), "load_ms": load_ms, "add_bases_ms": (time.perf_counter() - t0) * 1e3,
           "terms": {"fixed_base": 8, "variable_base": 10, "prepared_miller_pairs": 2}, "sizes": {}}
    rng = np.random.default_rng(2029)
    G = cc.Groth16
    val = lambda row: int.from_bytes(row.tobytes(), "little")
    for n in sizes:
        openings = _scalars(rng, 2 * n).reshape(n, 2, 32)
        openings[:, 0, max(nb // 8, 1):] = 0                           # m < 2^n_bits
        if nb < 8:
            openings[:, 0, 0] &= (1 << nb) - 1
        rand, c, rho, c_dleq = _scalars(rng, 18 * n).reshape(n, 18, 32), _scalars(rng, n), _scalars(rng, n), _scalars(rng, n)
        com_f, com_g, ts, st0 = G.range_commit_batch_packed(pk, pk_slot, openings, rand)
        com_q, _, st1 = G.range_quotient_batch_packed(pk, openings, rand, c)
        evals, proofs, st2 = G.range_open_batch_packed(pk, openings, rand, c, rho)
        assert all((s == cc.CG_SHOW_MADE).all() for s in (st0, st1, st2))
        pok_s = G.range_respond_batch(openings, rand, c_dleq)
        ped = com_g.copy()
        ped[0] = np.frombuffer(o.g1_uncompressed(RV.msm(bases, [val(openings[0, 0]), val(openings[0, 1])])), np.uint8)
        rz = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        call = lambda: G.range_verify_batch_packed(vk, slot, ped, com_f, com_g, com_q, evals, proofs, c, rho, rz, c_dleq, pok_s)
        verdicts, k = call()                                          # warm-up, buffer growth
        assert (verdicts == cc.CG_VERIFY_ACCEPT).all(), np.nonzero(verdicts != cc.CG_VERIFY_ACCEPT)[0][:8]
        assert (k == ts[:, 2:]).all() if n == 1 else (k[0] == ts[0, 2:]).all() and (k[:, 1] == ts[:, 3]).all()
        row0 = V.Row(ped[0].tobytes(), com_f[0].tobytes(), com_g[0].tobytes(), com_q[0].tobytes(), [val(e) for e in evals[0]],
                     [proofs[0, j, :64].tobytes() for j in range(3)], [val(proofs[0, j, 64:]) for j in range(3)], val(c[0]), val(rho[0]),
                     val(rz[0, :16]), val(rz[0, 16:]), val(c_dleq[0]), [val(s) for s in pok_s[0]])
        assert V.expected(K, bases, row0) == (V.ACCEPT, k[0].tobytes())
        runs = []
        for _ in range(a.reps):
            t = time.perf_counter()
            call()
            runs.append(((time.perf_counter() - t) * 1e3,) + vk.last_kernel_ms())
        runs.sort()
        mid = runs[len(runs) // 2]
        med = statistics.median(r[0] for r in runs)
        res["sizes"][str(n)] = {"median_ms": med, "min_ms": runs[0][0], "group_kernel_ms": mid[1], "pairing_kernel_ms": mid[2],
                                "ms_per_proof": med / n, "range_verifications_per_s": n / (med / 1e3)}
        if a.latency:                                                  # both arrangements, alternated call by call
            alt = {False: [], True: []}
            for mode in (False, True):
                vk.set_latency(mode)
                assert (call()[0] == cc.CG_VERIFY_ACCEPT).all()
            for _ in range(a.reps):
                for mode in (False, True):
                    vk.set_latency(mode)
                    t = time.perf_counter()
                    call()
                    alt[mode].append(((time.perf_counter() - t) * 1e3,) + vk.last_kernel_ms())
            vk.set_latency(False)
            for mode, name in ((False, "wide"), (True, "latency")):
                r = sorted(alt[mode])
                res["sizes"][str(n)][name] = {"median_ms": statistics.median(x[0] for x in r), "min_ms": r[0][0],
                                              "group_kernel_ms": r[len(r) // 2][1], "pairing_kernel_ms": r[len(r) // 2][2]}
            res["sizes"][str(n)]["wide_over_latency"] = res["sizes"][str(n)]["wide"]["median_ms"] / res["sizes"][str(n)]["latency"]["median_ms"]
    pk.close()
    vk.close()
    if not a.no_groth16:
        res["cg_verify_batch"] = {"ell": a.ell, "sizes": _groth16_yardstick(cc, a.ell, sizes, a.reps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
