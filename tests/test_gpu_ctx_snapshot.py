"""What cg_ctx_get_info reports of a context - the window of each of the five MSMs, the re-tune counters, the slots and the
resident bytes by kind - after the load, after one proof and after a second, against tests/golden/ctx_info_d12.json.  Needs an
MI355X.

Proof bytes cannot see a wrong window or a mis-booked buffer (an MSM gives the same point for any window), so the fixture holds
what the library reported before the prover's five queries were gathered into one set of tables and one set of engines: l's
digit statistics applied to a's table, or an engine left out of the byte count, shows here and nowhere else.

The fixture is recorded by this same body: CG_CTX_SNAPSHOT_RECORD=<path> writes the snapshots there instead of comparing them.
Recording over an existing file keeps, of the byte counts, the fields on which the two recordings agree; the other fields must
agree.  device_free_bytes / device_total_bytes are never kept.  Staged loads are left out: which proof's statistics the worker
sees depends on timing (tests/test_gpu_cold_start.py covers them by proof bytes)."""
import json
import os
import random

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "ctx_info_d12.json")
MANDATORY = ("window_bits", "tuned", "retune_attempts", "retune_skipped_for_memory", "proof_slots", "lone_slots", "latency_mode")
BYTES = ("table_bytes", "matrix_bytes", "slot_bytes", "slot_entry_bytes", "slot_piece_bytes", "slot_bucket_bytes", "slot_transform_bytes",
         "slot_upload_bytes", "lone_slot_bytes")

# name -> (Prover arguments, sharded, the first proof has r = 0)
CONTEXTS = {
    "throughput_3_slots_lone": (dict(proof_slots=3, mode="throughput"), False, False),
    "throughput_2_slots_no_lone": (dict(proof_slots=2, mode="throughput", lone_slot=False), False, False),
    "latency": (dict(mode="latency"), False, False),
    "window_bits_12": (dict(window_bits=12), False, False),
    "shard_0_of_2": (dict(shard_rank=0, shard_count=2), True, False),
    "shard_1_of_2": (dict(shard_rank=1, shard_count=2), True, False),
    "first_proof_r_zero": (dict(proof_slots=2, mode="throughput", lone_slot=False), False, True),
}


def _snapshot(prover):
    i = prover.info()
    return {k: i[k] for k in MANDATORY + BYTES}


def test_ctx_info_after_load_and_after_each_of_two_proofs(cc, oracle):
    from crescent_credentials_amd import workloads as wl
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()
    cm, w = wl.synthetic_circuit(812, 6, 4_000, 4_060, 0.9, 3)          # D = 2^12, a bit-heavy witness
    rng = random.Random(12)
    tau, alpha, beta, delta = (rng.randrange(1, oracle.R) for _ in range(4))
    pk = cc.generate_parameters_with_qap(cm, alpha, beta, delta, tau)
    r, s = 0x1234567890abcdef1234567890abcdef, 0xfedcba0987654321fedcba0987654321
    got, proofs = {}, {}
    for name, (kw, sharded, r_zero_first) in CONTEXTS.items():
        rs = [(0, s), (r, s)] if r_zero_first else [(r, s), (0, s)]
        p = cc.Prover(pk, cm, **kw)
        try:
            snaps = [_snapshot(p)]
            for rr, ss in rs:
                out = p.prove_partial(w, rr) if sharded else p.prove(w, rr, ss).data
                if not sharded:
                    assert proofs.setdefault((rr, ss), out) == out, name        # every arrangement proves the same bytes
                snaps.append(_snapshot(p))
        finally:
            p.close()
        print(name, json.dumps(snaps))
        got[name] = snaps
    # a proof with r = 0 skips b1: the re-tune gives b1's table the window of b2's, which has the same scalars
    wb = got["first_proof_r_zero"][1]["window_bits"]
    assert got["first_proof_r_zero"][1]["tuned"] == 1 and wb["b_g1"] == wb["b_g2"], wb

    record = os.environ.get("CG_CTX_SNAPSHOT_RECORD")
    if record:
        if os.path.exists(record):
            with open(record) as f:
                earlier = json.load(f)
            for name, snaps in got.items():
                for now, before in zip(snaps, earlier[name]):
                    for k in MANDATORY:
                        assert now[k] == before[k], (name, k, now[k], before[k])
                    for k in BYTES:
                        if k not in before or now[k] != before[k]:
                            print("not reproducible, dropped:", name, k, now[k], before.get(k))
                            now.pop(k)
        with open(record, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    with open(FIXTURE) as f:
        want = json.load(f)
    assert sorted(want) == sorted(got)
    for name, snaps in want.items():
        assert len(snaps) == 3
        for k, (now, before) in enumerate(zip(got[name], snaps)):
            assert all(f in before for f in MANDATORY), (name, k)
            assert {f: now[f] for f in before} == before, (name, k)
