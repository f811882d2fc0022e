"""bench.py --dump-outputs: the proof the last timed step returned, written as float arrays, the same in two runs with the
same arguments, and equal to the C restatement's proof on the inputs that step is documented to prove; and what a plain run
and a --full run put in the line."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _run(out_dir, steps, warmup):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--shape", "small", "--steps", str(steps), "--warmup",
           str(warmup), "--inflight", "4", "--headline-only", "--dump-outputs", out_dir]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    run = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [x for x in run.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, run.stdout[-2000:]
    d = json.loads(lines[0])
    proof = b"".join(bytes(np.load(os.path.join(out_dir, n + ".npy")).astype(np.uint8)) for n in ("proof_a", "proof_b", "proof_c"))
    return d, proof


def test_dump_outputs_is_the_last_timed_proof_and_repeats(cc, tmp_path):
    import cpu_ref
    from crescent_credentials_amd import workloads as wl
    steps, warmup = 7, 3
    d1, p1 = _run(str(tmp_path / "a"), steps, warmup)
    d2, p2 = _run(str(tmp_path / "b"), steps, warmup)
    for d in (d1, d2):
        assert d["steps"] == steps and d["timing"]["window_proofs"] == steps and d["timing"]["blocks"] == 5
        assert abs(d["ms_per_step"] * steps - d["timing"]["window_s"] * 1e3) < 0.01 * d["timing"]["window_s"] * 1e3 + 0.01
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["proof_a.npy", "proof_b.npy", "proof_c.npy"]
    assert p1 == p2 and len(p1) == 256
    # the same inputs made here, as bench.py makes them: seeded circuit and trapdoor, permuted assignments, step-keyed (r, s)
    R = cc.api.FR_MODULUS
    l, m, M = wl.SHAPES["small"]
    cm, w = wl.synthetic_circuit(0xC5E5CE47 + 3, l, m, M, 0.9, 3, profile="gates")
    trap_rng = random.Random(0xC5E5CE47)
    pk = cc.generate_parameters_with_qap(cm, *[trap_rng.randrange(1, R) for _ in range(4)])
    ws = bench.permuted_assignments(w, l, 4, 7)
    k = warmup + steps - 1
    r, s = bench.step_rs(k, 0, R)
    want = cpu_ref.prove(pk, (cm.a, cm.b, cm.c), l, m, M, ws[k % len(ws)], r, s, nthreads=8)
    assert p1 == want


FULL_ONLY = ("phase_ms", "roofline", "roofline_valu", "roofline_ntt", "legs_s", "proof_verifies", "key_check", "host_witness",
             "inflight_curve", "cold_start", "cpu_baseline", "shapes", "witness_sweep", "sharded")


def _line(extra, timeout=600):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--shape", "small", "--inflight", "4", *extra]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    run = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [x for x in run.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, run.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    """a plain run stops after the headline; --full measures and checks everything else on the same headline"""
    d = _line(["--steps", "6", "--warmup", "2"])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "timing", "config", "latency_ms"):
        assert k in d, k
    assert d["unit"] == "proofs/s" and d["higher_is_better"] is True and d["value"] > 0 and d["timing"]["window_proofs"] == 6
    assert "G1 MSM scalar-adds/sec reported alongside" in d["metric"]
    assert d["msm_g1_pairs_per_proof"] > 0                      # the line's value is rounded: the product agrees to its digits
    assert abs(d["g1_msm_scalar_adds_per_s"] - d["msm_g1_pairs_per_proof"] * d["value"]) <= 1e-4 * d["g1_msm_scalar_adds_per_s"]
    assert "bracketed" not in d["timing"] and not [k for k in FULL_ONLY if k in d]
    # the second shape (an S22 workload) is left out only to keep the test short
    f = _line(["--full", "--steps", "6", "--warmup", "2", "--no-shapes"], timeout=1200)
    assert f["timing"]["window_proofs"] == 6 and f["timing"]["bracketed"]["value"] > 0
    assert f["proof_verifies"] is True and f["key_check"]["ok"] is True and f["key_check"]["proof_equals_trapdoor_closed_form"] is True
    assert f["host_witness"]["bytes_identical_to_device_resident"] is True
    assert f["cold_start"]["proof_bytes_identical_to_the_resident_context"] is True
    assert f["cpu_baseline"]["proof_bytes_identical_to_gpu"] is True
    assert [p["in_flight"] for p in f["inflight_curve"]["points"]] == [1, 2, 4]
    assert len(f["witness_sweep"]) == 4 and f["phase_ms"]["total_ms"] > 0 and "roofline_valu" in f
    assert f["msm_g1_pairs_per_proof"] == d["msm_g1_pairs_per_proof"]
    assert set(f["legs_s"]) >= {"proof_check", "host_witness", "inflight_curve", "cold_start", "key_check", "cpu_baseline", "witness_sweep"}
