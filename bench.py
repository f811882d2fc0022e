#!/usr/bin/env python3
"""bench.py — Groth16 proofs/s (+ G1 MSM scalar-adds/s) of the HIP prove path on N MI355X.

Contract (driver):  python bench.py --gpus N --steps K --warmup W.  With N > 1 and no WORLD_SIZE in the environment
this process launches its own N ranks (python -m torch.distributed.run ..., before anything touches a GPU) and relays
rank 0's line and the exit code; launched under torch.distributed.run it is one of the ranks.  Rank 0 prints ONE JSON
line.

A "step" is one full Groth16 proof as SURVEY §8d defines the metric - witness in HOST memory -> 256-byte proof (cg_prove,
what creds/src/lib.rs:274-283 hands over): the 32·M-byte upload of the assignment from pageable memory, the witness map
(2 sparse products + 4 transforms with the folded key; 3 + 7 in the reference arrangement), four G1 MSMs, one G2 MSM and
the host finish, with fresh (r, s).  The same loop from page-locked memory (cg_host_alloc) and with the assignments
already resident in HBM (cg_prove_dev - rounds 1-4's headline) is measured beside it: `config.host_witness`,
`timing.device_resident`, `host_witness`.
Workload: the rs256-sd circuit's SHAPE (BASELINE.json metric; SURVEY.md §8d "S21": D = 2^21, m = 1 480 000,
M = 1 500 000, ℓ = 26), synthetic + satisfiable, ≈11 terms per row (nnz ≈ 16.6 M: the circomlib gate mix of
crescent-credentials_amd/synth/synth.cpp), with a proving key made by the GPU setup from a seeded trapdoor.  Real
Crescent circuits cannot be built in this environment.  The timed proofs rotate over several assignments of the same
value distribution, so that no step repeats the previous step's inputs.

Timed region.  Several proofs are in flight per GPU (that is how the latency-bound tails of one proof hide under the bulk
kernels of another), so a region of K proofs that starts and ends with an empty GPU contains a ramp-up and a drain that
weigh more the smaller K is (K = 20 with 12 in flight is 1.7 pipeline fills).  The headline is therefore measured in
steady state: after W warm-up proofs the stream of proofs keeps running and EXACTLY K consecutive completions are timed.
`value` = K proofs ÷ the time from the last warm-up completion to the K-th timed completion (max elapsed over ranks), and
`ms_per_step` is that time ÷ K.  For the block statistics the K completions are split into B consecutive blocks
(--blocks, default min(K, 5)); the median block (round 3's headline, which is biased high by up to 3 % on a bursty
stream: long blocks are the ones a median drops) is kept as `timing.median_block`, and the classical bracket (barrier +
synchronise, K proofs, synchronise + barrier; max over ranks) is measured in the same run and reported as
`timing.bracketed`.  The k-th proof of the headline stream proves assignment k mod --assignments with an (r, s) drawn
from a seed made of k and the rank, so the same arguments give the same inputs step for step in every run;
--dump-outputs DIR writes the proof of the last timed step as DIR/proof_{a,b,c}.npy.

Plain run and --full.  A plain run does what the headline needs and nothing more: it makes the workload and loads the key,
primes the proof slots, warms up, times the K steps, writes --dump-outputs and prints the line (metric, value, ms_per_step,
the block statistics and latencies of the same window, the configuration, and the G1 pair counts of one proof).  Every
other measurement and check - the bracketed region, the phase times and rooflines, the witness's other origins, the
in-flight curve, the cold start, the sharded proofs, the checker, the CPU baseline, the second shape and the bit-fraction
sweep - runs only with --full, as described below; the --no-* switches and --headline-only select among them there.

Multi-GPU: `value` is always the replica throughput — proofs are independent objects, each rank proves its
own stream with a full copy of the key, no data-path collective (config 5); `value_per_rank` lists every rank's own rate.
The CONTROL plane (barriers, max over ranks) always runs over gloo: the headline does not depend on RCCL coming up.  With
N > 1 the same run then measures proofs range-sharded over the ranks (cg_prove_partial, a 384-byte all_gather,
cg_assemble: config 4) - one at a time (latency) and several in flight per rank - and reports them as the `sharded`
sub-record (--full).  Only that leg opens an RCCL group, lazily, under the watchdog; if RCCL does not come up on every rank the
failure is recorded in `sharded.error` and the leg runs over gloo, labelled `backend_fallback`.

Checker (--full, rank 0, after the timed region; the oracle is never the thing measured): one proof taken from the TIMED stream
is verified by the Python oracle's pairing (`proof_verifies`, the reference's own acceptance criterion:
forks/groth16/src/test.rs:70-71, verifier.rs:44-65) and compared with the trapdoor's closed form, and the GPU-made key
the bench proves on is checked entry by entry against the trapdoor (`key_check`, oracle/keycheck.py).
"""
import argparse
import glob
import json
import math
import os
import random
import socket
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E (guides/MI355X_MICROARCH.md)
PEAK_CLOCK_GHZ = 2.4
N_SIMD = 256 * 4               # 256 CUs x 4 SIMDs
# The hardware's own figure (guides/MI355X_MICROARCH.md "Wave scheduling": CDNA4 SIMDs are 32 lanes wide, a wave64 VALU
# instruction issues in 2 cycles): 1228.8 G wave-instructions/s at 2.4 GHz - for the SIMPLE 32-bit instructions.  The
# multiply-adds this arithmetic is made of take twice that, so the honest utilisation is counted in SIMD CYCLES, each
# instruction class priced at what the SIMD measurably takes to issue it (tools/ubench/valu_rates --json, run inside this
# bench; round 5 read the rates from a committed text file and divided by a 4-cycle convention: kept as `legacy_*`).
VALU_PEAK_HW = N_SIMD * PEAK_CLOCK_GHZ * 1e9 / 2
VALU_PEAK = N_SIMD * PEAK_CLOCK_GHZ * 1e9 / 4   # legacy: one VALU instruction per 4 cycles (the SIMD-16 model of rounds 1-5)
# What the vector ALU really issues (round 5, tools/ubench/valu_rates.hip -> profiles/r05_e_valu_issue_rates.txt, cycles per
# wave-instruction per SIMD): the 64-bit multiply-add the limb products are made of takes 4.91 - not the 4 the nominal peak
# assumes - other VOP3 / 64-bit integer operations 4.5, and simple 32-bit VOP1/VOP2 operations (mov, and, add, sub, shifts)
# 2.5.  With the static mix of the hot loops (G1 mixed addition 72 / 14 / 14 %, butterflies 68 / 21 / 11 %: ~70 % multiply-adds,
# ~16 % simple, ~14 % other) an instruction of this workload costs 4.47 cycles: the ceiling is 0.895 of the nominal peak.
ISSUE_CYCLES = {"mad64": 4.91, "other": 4.5, "simple32": 2.5}
ISSUE_MIX = {"mad64": 0.70, "other": 0.14, "simple32": 0.16}
MIX_CYCLES = sum(ISSUE_CYCLES[k] * ISSUE_MIX[k] for k in ISSUE_MIX)
G1_PAIR_BYTES = 96             # 64 B affine base + 32 B scalar   
G2_PAIR_BYTES = 160
SWEEP_FRACTIONS = (0.0, 0.5, 0.75, 0.9)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--shape", default=None,
                    help="the headline workload's shape (crescent-credentials_amd/workloads.py SHAPES); default rs256-sd, the configuration "
                         "BASELINE.json's metric is quoted on")
    ap.add_argument("--sharded-shape", default=None,
                    help="N > 1: the shape the SHARDED proofs are made on; default mdl1 (S22: BASELINE.json's config 4 is 'mdl1 ... MSM sharded "
                         "across 8 x MI355X') unless --shape was given, in which case that shape")
    ap.add_argument("--bits", type=float, default=0.9,
                    help="share of the aux wires that are bit gates' outputs in the headline workload (see DESIGN.md §5)")
    ap.add_argument("--profile", default="gates", choices=["gates", "r1"],
                    help="synthetic matrix mix: gates = circomlib gate mix, ~11 terms per row (SURVEY 8d); r1 = round 1's "
                         "booleanity + short product rows, ~3.4 terms per row (kept for A/B against round-1 numbers)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-sweep", action="store_true", help="skip the secondary witness_sweep measurements")
    ap.add_argument("--no-host-witness", action="store_true",
                    help="skip the secondary legs of the witness's origin (page-locked host memory, device-resident)")
    ap.add_argument("--witness", default="host", choices=["host", "pinned", "device"],
                    help="where the timed proofs' assignments come from: host = pageable host memory through cg_prove (the metric as "
                         "SURVEY 8d writes it, the default), pinned = page-locked host memory, device = already in HBM (cg_prove_dev: "
                         "profiling runs, A/B of kernels)")
    ap.add_argument("--mode", default=None, choices=["latency", "throughput"],
                    help="force the context's arrangement (CG_FLAG_LATENCY_MODE / CG_FLAG_THROUGHPUT_MODE); default: proof slots decide. "
                         "`--inflight 1 --mode throughput` is the profiling arrangement: one proof at a time on one stream with the "
                         "pipelined run's kernels")
    ap.add_argument("--no-sharded", action="store_true", help="N > 1: skip the sharded-proof sub-record")
    ap.add_argument("--sharded-steps", type=int, default=20, help="N > 1: sharded proofs timed one at a time (latency)")
    ap.add_argument("--sharded-inflight", type=int, default=8,
                    help="N > 1: sharded proofs kept in flight per rank in the pipelined leg (two ranks on one GPU: 142.5 proofs/s with "
                         "4, 159.0 with 8, against 116.5 one at a time and 196 for replicas: profiles/r04_h_*, r04_i_sharded_inflight8.txt)")
    ap.add_argument("--sharded-stream", type=int, default=160, help="N > 1: sharded proofs of the pipelined leg")
    ap.add_argument("--rccl-deadline", type=float, default=90.0,
                    help="N > 1: seconds the RCCL data group may take to come up (creation + first all_gather) before the sharded leg "
                         "falls back to gloo")
    ap.add_argument("--strict-exit", action="store_true",
                    help="N > 1: when the watchdog has to print the line, rank 0 leaves with exit code 4 as well (default: rank 0 prints the "
                         "line marked `incomplete` and exits 0, every OTHER rank exits 4 five seconds later - the launcher's return code says "
                         "that the run did not complete, and the line is on stdout by then)")
    ap.add_argument("--no-check", action="store_true", help="skip the checker leg (proof_verifies, key_check)")
    ap.add_argument("--no-cold-start", action="store_true",
                    help="skip the cold_start record (the reference's own call: main_c.r1cs + prover_params.bin -> client_state.bin "
                         "through the compiled C caller, with the CPU restatement's chain beside it)")
    ap.add_argument("--no-shapes", action="store_true", help="N = 1: skip the second-shape record (`shapes`: mdl1 / S22, SURVEY 8d 'report both')")
    ap.add_argument("--no-latency-curve", action="store_true", help="skip `inflight_curve` (rate and latency at 1 / 2 / 4 / 8 / 16 proofs in flight)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, every other measurement and check: the bracketed region, phase times and rooflines, the "
                         "secondary legs (host witness, latency curve, cold start, sharded proofs, CPU baseline, second shape, sweep) and "
                         "the checker.  Without it the run stops after the headline; the --no-* switches act on a --full run")
    ap.add_argument("--headline-only", action="store_true",
                    help="with --full: the headline, the bracketed region, the phase times and the rooflines that need no run of their "
                         "own, and nothing else (implies every --no-* leg switch: sweep, CPU baseline, host witness, checker, cold start, "
                         "shapes, latency curve, micro-benchmark, sharded leg).  Without --full it changes nothing")
    ap.add_argument("--no-ubench", action="store_true", help="do not run tools/ubench/valu_rates (the in-run VALU issue rates of `roofline_valu`)")
    ap.add_argument("--stall-rank", type=int, default=-1,
                    help="testing aid: this rank stops before the sharded leg, as a rank that failed alone would (exercises --leg-timeout)")
    ap.add_argument("--leg-timeout", type=int, default=300,
                    help="N > 1: seconds the secondary legs (host witness, sharded proof) may take before rank 0 prints the line "
                         "it has and every rank leaves (0 = no watchdog)")
    ap.add_argument("--shard-sim", type=int, default=0,
                    help="N = 1 only: time one proof split over this many sharded contexts on the one GPU, shard by shard")
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--h-coefficient-basis", action="store_true",
                    help="keep the h query as loaded and run the seventh transform per proof (A/B against the default)")
    ap.add_argument("--backend", default="nccl",
                    help="N > 1: backend of the DATA plane (the sharded leg's 384-byte all_gather): nccl = RCCL, gloo for plumbing tests; "
                         "the control plane is always gloo")
    ap.add_argument("--allow-shared-gpu", action="store_true",
                    help="N > visible GPUs: let several ranks share a GPU (implied by --backend gloo; RCCL needs a GPU per rank)")
    ap.add_argument("--inflight", type=int, default=16,
                    help="proofs in flight per GPU: host threads x context proof_slots, one stream each.  Round 4 (70 launches per proof): "
                         "6: 177.5, 8: 188.7, 10: 191.6, 12: 196.8, 16: 196.8 proofs/s on one box (profiles/r04_m_inflight_low.txt) - twelve "
                         "give the rate of sixteen with a quarter less memory and time in the pipeline per proof; round 3 (84 launches) "
                         "needed sixteen (8: 185, 12: 194, 16: 197).  Round 5, with the witness arriving in HOST memory (the headline): the "
                         "upload adds to a proof's time in flight and sixteen are worth +1 % again: 10: 192.9, 12: 196.3, 16: 198.2 "
                         "(profiles/r05_i_inflight_and_tiles.txt; 28.9 GB resident)")
    ap.add_argument("--assignments", type=int, default=4, help="device-resident assignments the timed proofs rotate over")
    ap.add_argument("--no-clock-probe", action="store_true",
                    help="do not sample the shader clock during the timed proofs (profiling runs: under rocprofv3 --pmc kernels "
                         "are serialised and the probe's sleeping wave would hold the others up)")
    ap.add_argument("--blocks", type=int, default=0,
                    help="consecutive blocks the --steps timed proofs are split into for the block statistics (0 = min(steps, 5))")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the proof the last timed step returned as DIR/proof_a.npy, proof_b.npy, proof_c.npy (its 64 / 128 / 64 "
                         "ark-serialize uncompressed bytes as float64 values 0..255), on rank 0")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return a


def visible_gpus_without_hip() -> int:
    """GPUs this process will see, counted without initialising the HIP runtime (which reads GPU_MAX_HW_QUEUES once, when
    it starts): the *_VISIBLE_DEVICES list if there is one, else the KFD topology nodes that have SIMDs.  0 = unknown."""
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None and v.strip():
            return len([x for x in v.split(",") if x.strip()])
    n = 0
    for f in glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties"):
        try:
            with open(f) as fh:
                for line in fh:
                    if line.startswith("simd_count "):
                        n += int(line.split()[1]) > 0
        except (OSError, ValueError):
            pass
    # a container that was given some of the host's GPUs has only their render nodes (the pool's one-GPU boxes: ten topology
    # nodes, one of them readable, one /dev/dri/renderD*)
    r = sum(1 for p in glob.glob("/dev/dri/renderD*") if os.access(p, os.R_OK | os.W_OK))
    return min(n, r) if n and r else (n or r)


def self_launch(a) -> int:
    """`--gpus N` without a launcher: start the N ranks as fresh child processes.  Nothing in this parent has touched a
    GPU (counting devices does not, on this image), so the children are not an exec from a GPU-initialised process."""
    import torch
    ndev = torch.cuda.device_count()
    if ndev == 0:
        print("bench.py: no GPU visible", file=sys.stderr)
        return 2
    if a.gpus > ndev and not (a.allow_shared_gpu or a.backend == "gloo"):
        print("bench.py: --gpus %d but %d GPU(s) visible: RCCL needs one GPU per rank.  For a plumbing run with ranks "
              "sharing a GPU use --backend gloo (or --allow-shared-gpu)." % (a.gpus, ndev), file=sys.stderr)
        return 2
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(launch_command(a.gpus, sys.argv[1:]), env=env).returncode


def launch_command(n_ranks, argv, port=None):
    """the driver's own multi-GPU command line (one rank per GPU, rendezvous on 127.0.0.1) around this script"""
    if port is None:
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks),
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def committed_counters(workload_key):
    """rocprofv3 PMC results cannot be read from inside this process; the figures come from the committed passes in
    profiles/pmc_counters.json (separate --pmc runs of THIS command, FETCH_SIZE / WRITE_SIZE corrected as
    guides/MI355X_MICROARCH.md prescribes, SQ_INSTS_VALU per steady-state proof), keyed by workload and stamped with the
    fingerprint of the kernel sources they were taken on.  -> (entry or None, fingerprint matches this tree)"""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_counters.json")) as f:
            e = json.load(f).get(workload_key)
    except Exception:
        return None, False
    if not e:
        return None, False
    return e, e.get("csrc_sha16") == source_fingerprint()


def source_fingerprint():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cg_build", os.path.join(ROOT, "crescent-credentials_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.source_fingerprint()


def permuted_assignments(w_np, l, count, seed):
    """the satisfying witness plus `count - 1` assignments with its aux wires permuted: the same multiset of values
    (hence the same digit statistics) in other positions.  The prover's cost does not depend on satisfaction."""
    import numpy as np
    out = [w_np]
    W = w_np.reshape(-1, 32)
    rng = np.random.default_rng(seed)
    for _ in range(count - 1):
        p = W.copy()
        p[l:] = W[l:][rng.permutation(W.shape[0] - l)]
        out.append(p.reshape(-1).copy())
    return out


class ClockSampler:
    """samples the shader clock on the device (cg_probe_shader_clock: one sleeping wave, 20 ms windows) from a side thread
    while the timed proofs run"""

    def __init__(self, cc, device):
        self.cc, self.device, self.samples, self._stop = cc, device, [], threading.Event()
        self._t = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        while not self._stop.is_set():
            try:
                self.samples.append(self.cc.probe_shader_clock(self.device, 20000))
            except Exception:
                return
            self._stop.wait(0.05)

    def __enter__(self):
        self._t.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._t.join(timeout=5)

    def median(self):
        s = sorted(self.samples)
        return round(s[len(s) // 2], 3) if s else None


def steady_stream(prove_one, total, inflight, latencies=None):
    """`total` calls of prove_one(k), `inflight` at a time from as many host threads, never letting the pipeline run
    dry; returns the sorted completion times.  latencies (a list, optional) receives (completion time, seconds the call
    took) of every proof: what ONE caller waited for its proof."""
    done = [0.0] * total
    began = [0.0] * total
    nxt = [0]
    lock = threading.Lock()
    err = []

    def worker():
        while not err:
            with lock:
                k = nxt[0]
                nxt[0] += 1
            if k >= total:
                return
            began[k] = time.perf_counter()
            try:
                prove_one(k)
            except BaseException as e:   # surfaces below
                err.append(e)
                return
            done[k] = time.perf_counter()
    ts = [threading.Thread(target=worker) for _ in range(max(1, min(inflight, total)))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if err:
        raise err[0]
    if latencies is not None:
        latencies.extend(sorted((done[k], done[k] - began[k]) for k in range(total)))
    return sorted(done)


def percentiles_ms(xs):
    """{p50, p95, p99, max} of a list of seconds, in ms"""
    s_ = sorted(xs)
    if not s_:
        return None
    at = lambda q: s_[min(len(s_) - 1, int(q * len(s_)))]
    return {"p50": round(at(0.50) * 1e3, 3), "p95": round(at(0.95) * 1e3, 3), "p99": round(at(0.99) * 1e3, 3), "max": round(s_[-1] * 1e3, 3)}


def cold_start_record(cc, a, pk, cm, w_np, l, m, M, fresh_rs, prover, ws_dev, log):
    """The reference's own call at the reference's artefact size, in a FRESH process: `create_client_state`
    (creds/src/lib.rs:255-301: read main_c.r1cs, read prover_params.bin, prove once, write client_state.bin) through the compiled
    C caller integration/c/crescent_prove, which sees nothing but include/crescent_gpu.h.  The input files are written here from
    the headline workload (oracle-side writers: fixtures, not the thing measured); the caller's own phase clock is the record.
    The same files are then read by the C restatement's readers (the CPU chain's parse; its proof is timed by the cpu_baseline
    leg and joined there)."""
    import shutil
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ark_files
    import bn254_oracle as o
    import cpu_ref
    import numpy as np
    exe = os.path.join(ROOT, "integration", "c", "crescent_prove")
    tmp = tempfile.mkdtemp(prefix="cg_cold_start_")
    try:
        t0 = time.perf_counter()
        f = {k: os.path.join(tmp, k) for k in ("main_c.r1cs", "prover_params.bin", "witness.bin", "client_state.bin")}
        cpu_ref.write_r1cs((cm.a, cm.b, cm.c), m, M, 2, l - 3, M - l).tofile(f["main_c.r1cs"])
        g1 = lambda x: o.g1_unpack(bytes(x))
        g2 = lambda x: o.g2_unpack(bytes(x))
        vk = pk.vk
        ovk = dict(alpha_g1=g1(vk.alpha_g1), beta_g2=g2(vk.beta_g2), gamma_g2=g2(vk.gamma_g2), delta_g1=g1(vk.delta_g1), delta_g2=g2(vk.delta_g2),
                   gamma_abc_g1=[g1(vk.gamma_abc_g1[64 * i:64 * i + 64]) for i in range(vk.gamma_abc_g1.size // 64)])
        pvk = ark_files.prepare_verifying_key(ovk)                      # Groth16::process_vk (creds/src/lib.rs:232)
        cfg = b'{"alg": "RS256", "exp": {"type": "number", "reveal": true, "max_claim_byte_len": 31}}'
        with open(f["prover_params.bin"], "wb") as fh:                  # ProverParams = key | prepared key | config (lib.rs:58-63)
            cpu_ref.write_pk(pk, nthreads=cpu_ref.best_threads()).tofile(fh)
            fh.write(ark_files.pvk_bytes(pvk))
            fh.write(len(cfg).to_bytes(8, "little") + cfg)
        w_np.tofile(f["witness.bin"])
        made_s = time.perf_counter() - t0
        r_, s_ = fresh_rs()

        def run(extra=()):
            cmd = [exe, f["main_c.r1cs"], f["prover_params.bin"], f["witness.bin"], f["client_state.bin"], "--rs", "%x" % r_, "%x" % s_,
                   "--timings-json", *extra]
            t1 = time.perf_counter()
            pr = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            wall = time.perf_counter() - t1
            if pr.returncode != 0:
                raise RuntimeError("crescent_prove failed: " + pr.stderr[-1500:])
            rec_ = json.loads(pr.stdout.strip().splitlines()[-1])
            proof_ = cc.ClientState.from_bytes(open(f["client_state.bin"], "rb").read()).proof.data
            return rec_, proof_, wall
        want = prover.prove_dev(ws_dev[0].data_ptr(), r_, s_).data     # ws_dev[0] is w_np
        staged, p_staged, wall_staged = run()
        sync, p_sync, _ = run(("--sync-load",))
        same = p_staged == want and p_sync == want
        # the CPU chain's share of reading: the C restatement's own readers on the same two files
        t1 = time.perf_counter()
        hdr, mats = cpu_ref.read_r1cs(np.fromfile(f["main_c.r1cs"], np.uint8))
        cpu_r1cs_s = time.perf_counter() - t1
        t1 = time.perf_counter()
        pk2, _used = cpu_ref.read_pk(np.fromfile(f["prover_params.bin"], np.uint8), nthreads=cpu_ref.best_threads())
        cpu_pp_s = time.perf_counter() - t1
        parsed_ok = (all(np.array_equal(x.col, y.col) and np.array_equal(x.coeff, y.coeff) for x, y in zip(mats, (cm.a, cm.b, cm.c)))
                     and np.array_equal(pk2.h_query, pk.h_query) and np.array_equal(pk2.b_g2_query, pk.b_g2_query))
        gb = lambda n_, s__: round(n_ / s__ / 1e9, 2) if s__ > 0 else None
        rec = {
            "what": "files -> client_state.bin in a fresh process: integration/c/crescent_prove (strict C11 over include/crescent_gpu.h), "
                    "staged load (CG_FLAG_STAGED_LOAD), ONE proof - the reference's create_client_state (creds/src/lib.rs:255-301)",
            "workload": "%s: main_c.r1cs %d bytes, prover_params.bin %d bytes" % (a.shape, staged["r1cs_bytes"], staged["prover_params_bytes"]),
            # the reference's own timers (creds/src/lib.rs:257,266,281) and what stands for them here
            "reading_r1cs_s": round(staged["r1cs_read_s"] + staged["r1cs_parse_s"], 4),
            "reading_prover_params_s": round(staged["prover_params_read_s"] + staged["prover_params_parse_s"], 4),
            "r1cs_parse_s": staged["r1cs_parse_s"], "prover_params_parse_s": staged["prover_params_parse_s"],
            "r1cs_parse_GB_per_s": gb(staged["r1cs_bytes"], staged["r1cs_parse_s"]),
            "prover_params_parse_GB_per_s": gb(staged["prover_params_bytes"], staged["prover_params_parse_s"]),
            "gpu_runtime_init_and_witness_read_s": staged["gpu_init_and_witness_s"],
            "files_parsed_after_s": staged["files_parsed_after_s"],
            "circuit_load_s": staged["circuit_load_s"], "circuit_load_split_ms": staged["circuit_load_split_ms"],
            "first_proof_ms": staged["first_proof_ms"], "groth16_prove_s": round(staged["first_proof_ms"] / 1e3, 4),
            "total_s": staged["total_s"], "process_wall_s_incl_background_and_exit": round(wall_staged, 3),
            "background": dict(staged["background"], second_proof_ms=staged["second_proof_ms"],
                               note="built by the library's worker behind the first proof: the h query's change of basis, the per-window "
                                    "tables, the final proof slots; the context then proves at the steady rate"),
            "synchronous_load": {"circuit_load_s": sync["circuit_load_s"], "circuit_load_split_ms": sync["circuit_load_split_ms"],
                                 "first_proof_ms": sync["first_proof_ms"], "total_s": sync["total_s"]},
            "proof_bytes_identical_to_the_resident_context": bool(same),
            "cpu_chain": {"reading_r1cs_s": round(cpu_r1cs_s, 3), "reading_prover_params_s": round(cpu_pp_s, 3),
                          "readers": "oracle/cpu_ref.c ref_r1cs_scan/_fill (one thread, as R1CSFile::new reads) and ref_pk_scan/ref_points_strip",
                          "parsed_arrays_identical_to_the_source": bool(parsed_ok)},
            "input_files_made_in_s": round(made_s, 1),
        }
        log("cold start: files -> client_state.bin in %.3f s (load %.3f s, first proof %.1f ms); synchronous load %.3f s" %
            (staged["total_s"], staged["circuit_load_s"], staged["first_proof_ms"], sync["total_s"]))
        assert same, "the cold-start proof differs from the resident context's"
        assert parsed_ok, "the CPU readers and the source arrays differ"
        return rec
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def block_times(done, warmup, n_timed, blocks, t_start):
    """seconds per proof of each of the `blocks` consecutive blocks that the `n_timed` completions after the first `warmup`
    completions are split into (block sizes differ by at most one)"""
    edge = lambda i: done[i - 1] if i > 0 else t_start
    e = [warmup + b * n_timed // blocks for b in range(blocks + 1)]
    return [(edge(e[b + 1]) - edge(e[b])) / (e[b + 1] - e[b]) for b in range(blocks)]


def n_blocks(a):
    """blocks the headline's window of exactly --steps proofs is split into for the block statistics"""
    return max(1, min(a.blocks if a.blocks > 0 else 5, a.steps))


def step_rs(k, rank, modulus):
    """(r, s) of the k-th proof of the headline stream: drawn from a seed made of k and the rank, whichever caller thread
    takes proof k, so that a step proves the same inputs in every run with the same arguments"""
    g = random.Random(((1234 + rank) << 32) | k)
    return g.randrange(modulus), g.randrange(modulus)


def dump_proof(out_dir, data):
    """a proof's 256 bytes (a | b | c, ark-serialize uncompressed) as DIR/proof_{a,b,c}.npy, float64 byte values"""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    b = np.frombuffer(bytes(data), dtype=np.uint8).astype(np.float64)
    for name, part in (("proof_a", b[:64]), ("proof_b", b[64:192]), ("proof_c", b[192:])):
        np.save(os.path.join(out_dir, name + ".npy"), part)


def main():
    a = parse()
    if a.headline_only:
        a.no_sweep = a.no_cpu_baseline = a.no_host_witness = a.no_check = a.no_cold_start = a.no_shapes = a.no_latency_curve = True
        a.no_ubench = a.no_sharded = True
    a.sharded_shape = a.sharded_shape or (a.shape if a.shape else "mdl1")
    a.shape = a.shape or "rs256-sd"
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(a))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # Several proofs are kept in flight per GPU, one HIP stream each; the runtime maps streams onto this many hardware queues
    # (default 4), and kernels of streams that share a queue cannot overlap.  More than ~24 user queues per GPU and the
    # hardware scheduler time-slices them (15 ms stalls for a lone proof or a shard), so ranks that share a GPU (plumbing
    # runs) split the budget.  Must be set before the HIP runtime initialises.
    # (Counted without a torch device call: should torch ever count devices through hipGetDeviceCount, the runtime would
    # have read its flags before the variable is set.)
    ndev = visible_gpus_without_hip()
    if ndev == 0:
        import torch
        ndev = max(1, torch.cuda.device_count())
    ranks_per_gpu = max(1, math.ceil(int(os.environ.get("LOCAL_WORLD_SIZE", world)) / ndev))
    # (eight plumbing ranks on one GPU get two queues each: 8 x 4 = 32 user queues would be above the ~24 at which the hardware
    # scheduler starts time-slicing)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", str(20 if ranks_per_gpu == 1 else max(2, 16 // ranks_per_gpu)))
    # the RCCL group of the sharded leg must never take the process down: no asynchronous tear-down on a failed or
    # timed-out collective, no heartbeat monitor (the leg has its own deadline and falls back to gloo)
    os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "0")
    os.environ.setdefault("TORCH_NCCL_ENABLE_MONITORING", "0")
    import torch
    import numpy as np
    import torch.distributed as dist

    # the contract is ONE JSON line on stdout: whatever the runtime libraries print there on the way (gloo's connection
    # banner, for one) is sent to stderr instead; stdout is restored for the line itself
    sys.stdout.flush()
    stdout_fd = os.dup(1)
    os.dup2(2, 1)
    assert torch.cuda.is_available(), "bench.py needs a GPU (there is no CPU path to measure)"
    local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("gloo")        # the control plane; RCCL is opened by the sharded leg only (open_data_group)

    import crescent_credentials_amd as cc
    from crescent_credentials_amd import workloads as wl
    from crescent_credentials_amd.distributed import (ShardedProver, barrier_sync, gather_over_ranks, max_over_ranks,
                                                      open_data_group)

    assert cc.lib().cg_init(0, None) == 0, cc.lib().cg_last_error()
    cc.set_device(local_rank)          # the key generation below has no device argument (the library's runtime is not torch's)
    R = cc.api.FR_MODULUS
    l, m, M = wl.SHAPES[a.shape]
    log = (lambda *x: print("[bench]", *x, file=sys.stderr, flush=True)) if rank == 0 else (lambda *x: None)
    inflight = max(1, a.inflight)
    rs_rng = random.Random(1234 + rank)
    rs_lock = threading.Lock()
    trap_rng = random.Random(0xC5E5CE47)
    trap = [trap_rng.randrange(1, R) for _ in range(4)]

    def fresh_rs():
        with rs_lock:
            return rs_rng.randrange(R), rs_rng.randrange(R)

    keyed_rs = lambda k: step_rs(k, rank, R)

    def emit(out_):
        """rank 0 prints the line on the real stdout; then a multi-rank run's process group comes down"""
        sys.stdout.flush()
        os.dup2(stdout_fd, 1)
        if rank == 0:
            print(json.dumps(out_), flush=True)
        if world > 1:
            os.dup2(2, 1)
            # the line is out: a process group that does not come down must not keep the ranks (and the driver) waiting
            t_exit = threading.Timer(30, lambda: os._exit(0))
            t_exit.daemon = True
            t_exit.start()
            dist.destroy_process_group()

    def make_workload(bits, seed_off, dims=None):
        l_, m_, M_ = dims or (l, m, M)
        cm_, w_ = wl.synthetic_circuit(0xC5E5CE47 + seed_off, l_, m_, M_, bits, 3, profile=a.profile)
        pk_ = cc.generate_parameters_with_qap(cm_, *trap)
        return cm_, w_, pk_

    def prime(prove_k):
        """the one-time window re-tune that follows a context's first proof belongs to circuit loading, and every proof
        slot captures its reduction graphs on first use: both happen before the W warm-up steps"""
        prove_k(0)
        steady_stream(prove_k, inflight, inflight)
        torch.cuda.synchronize()

    def measure(prove_k, n_timed, warmup, blocks, sync_ranks, clock=None, threads=None):
        """-> (seconds of the steady window of n_timed proofs [max over ranks], record, every rank's own proofs/s); the window
        is split into `blocks` consecutive blocks for the block statistics.  prove_k(k): the k-th proof of the stream."""
        threads = threads or inflight
        total = warmup + n_timed + threads                   # the tail keeps the end of the window in steady state
        if sync_ranks:
            barrier_sync(world)
        t_start = time.perf_counter()
        cpu0 = time.process_time()
        lat = []
        if clock is not None:
            with clock:
                done = steady_stream(prove_k, total, threads, lat)
        else:
            done = steady_stream(prove_k, total, threads, lat)
        cpu_busy = (time.process_time() - cpu0) / max(1e-9, time.perf_counter() - t_start)
        torch.cuda.synchronize()
        window = done[warmup + n_timed - 1] - (done[warmup - 1] if warmup > 0 else t_start)
        bt = sorted(block_times(done, warmup, n_timed, blocks, t_start))      # seconds per proof of each block
        med = bt[len(bt) // 2]
        per_block = n_timed / blocks
        rec = {"window_proofs": n_timed, "window_s": round(window, 4), "blocks": blocks,
               "median_block": {"ms_per_step": round(med * 1e3, 3), "value_this_rank": round(1.0 / med, 3),
                                "spread_pct": round((bt[-1] - bt[0]) / med * 100.0, 2),
                                "block_ms_min_median_max": [round(x * per_block * 1e3, 2) for x in (bt[0], med, bt[-1])]},
               "host_cpus_busy": round(cpu_busy, 2),     # process CPU seconds per second of the stream: what the callers cost the host
               # what ONE caller waits for its proof inside this stream (call to return of cg_prove*, the proofs of the timed window)
               "latency_ms": percentiles_ms([d for t_, d in lat if (done[warmup - 1] if warmup > 0 else t_start) < t_ <= done[warmup + n_timed - 1]])}
        per_rank = [n_timed / window]
        if sync_ranks:
            barrier_sync(world)
            per_rank = gather_over_ranks(n_timed / window, world)
            window = max_over_ranks(window, world)
        return window, rec, per_rank

    def bracketed(prove_k, steps, sync_ranks, threads=None):
        """the classical region: empty GPU, K proofs, empty GPU"""
        if sync_ranks:
            barrier_sync(world)
        else:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        steady_stream(prove_k, steps, threads or inflight)
        torch.cuda.synchronize()
        if sync_ranks:
            barrier_sync(world)
        dt = time.perf_counter() - t0
        return max_over_ranks(dt, world) if sync_ranks else dt

    def phase_record(prover, w_dev, reps=3):
        accs = [prover.prove_dev(w_dev.data_ptr(), *fresh_rs(), timings=True)[1] for _ in range(reps)]
        keys = ("witness_map_ms", "msm_h_ms", "msm_l_ms", "msm_a_ms", "msm_b1_ms", "msm_b2_ms", "sort_ms", "accum_g1_ms",
                "accum_g2_ms", "finish_ms", "total_ms")
        return accs[-1], {k: round(float(np.mean([t[k] for t in accs])), 3) for k in keys}

    # ---- headline workload (identical on every rank: same seeds) ----------------------------------
    t0 = time.time()
    cm, w_np, pk = make_workload(a.bits, 3)
    nnz = cm.a.nnz + cm.b.nnz + cm.c.nnz
    wires = wl.wire_stats(w_np)
    log("workload %s: l=%d m=%d M=%d nnz=%d wires=%s, key + circuit made in %.1fs" % (a.shape, l, m, M, nnz, wires, time.time() - t0))
    t0 = time.time()
    prover = cc.Prover(pk, cm, device=local_rank, window_bits=a.window, proof_slots=inflight, h_coefficient_basis=a.h_coefficient_basis,
                       mode=a.mode)
    log("circuit loaded on GPU in %.1fs (D = %d)" % (time.time() - t0, prover.domain_size))
    ws_np = permuted_assignments(w_np, l, max(1, a.assignments), 7)
    ws_dev = [torch.from_numpy(x).to(dev) for x in ws_np]
    torch.cuda.synchronize()

    timed_sample = {}       # the latest proof the stream made on the SATISFYING assignment (the permuted ones satisfy nothing)
    pinned = []             # page-locked copies of the assignments (cg_host_alloc), made on first use

    def pinned_buffers():
        if not pinned:
            for x in ws_np:
                hb = cc.HostBuffer(x.size)
                hb.array[:] = x
                pinned.append(hb)
        return pinned

    def stream_of(origin, sample=None, keep=None):
        """prove_k(k) for assignments arriving from `origin`: 'host' = pageable host memory (numpy arrays) through cg_prove,
        'pinned' = page-locked host memory through cg_prove, 'device' = already in HBM through cg_prove_dev.  With `keep`
        (the headline stream) (r, s) is keyed_rs(k), and the proof of step keep["k"] is kept as keep["proof"]."""
        if origin == "pinned":
            pinned_buffers()

        def prove_k(k):
            j = k % len(ws_np)
            r_, s_ = keyed_rs(k) if keep is not None else fresh_rs()
            if origin == "host":
                p = prover.prove_host_ptr(ws_np[j].ctypes.data, r_, s_)
            elif origin == "pinned":
                p = prover.prove_host_ptr(pinned[j].ptr, r_, s_)
            else:
                p = prover.prove_dev(ws_dev[j].data_ptr(), r_, s_)
            if sample is not None and j == 0:
                sample["proof"] = (k, r_, s_, p.data)
            if keep is not None and k == keep.get("k"):
                keep["proof"] = p.data
        return prove_k

    # two more caller threads than proof slots when the witness arrives from the host: a context holds that many more upload
    # buffers, so the next assignments arrive while every working set is busy
    callers_of = lambda origin: inflight if origin == "device" else inflight + 2
    last_step = {}          # the proof of the last timed step (--dump-outputs)
    prove_headline_k = stream_of(a.witness, timed_sample, last_step)
    callers = callers_of(a.witness)

    blocks = n_blocks(a)
    n_timed = a.steps
    prime(prove_headline_k)
    clock = ClockSampler(cc, local_rank) if rank == 0 and not a.no_clock_probe else None
    last_step["k"] = a.warmup + n_timed - 1             # proof number of the last timed step in the measured stream
    dt, timing, per_rank = measure(prove_headline_k, n_timed, a.warmup, blocks, True, clock, threads=callers)
    last_step.pop("k")
    value = n_timed * world / dt
    checked_proof = timed_sample.get("proof")           # taken before any later leg overwrites it
    if a.dump_outputs and rank == 0:
        dump_proof(a.dump_outputs, last_step["proof"])
    info = prover.info()
    out = {
        "metric": "Groth16 proofs/sec (rs256-sd-shaped circuit, BN254), G1 MSM scalar-adds/sec reported alongside",
        "value": round(value, 3), "unit": "proofs/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(dt / n_timed * 1e3, 4), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "u32 limbs (BN254 Fq/Fr, 254-bit modular integers)",
        "data": "synthetic",
        "value_per_rank": [round(x, 3) for x in per_rank],
        "timing": dict(timing, method="steady state: `steps` consecutive proof completions with the pipeline kept primed, split into "
                                      "`blocks` blocks for the block statistics; value = proofs / elapsed over that whole window "
                                      "(max elapsed over ranks)"),
        "config": {"workload": "%s shape: D=2^%d, m=%d, M=%d, l=%d, nnz=%d (%s mix); bit_fraction=%.2f; pk from seeded trapdoor (GPU setup)" %
                   (a.shape, prover.domain_size.bit_length() - 1, m, M, l, nnz, a.profile, a.bits),
                   "wires": wires, "mode": "throughput (one full key replica per GPU)",
                   "baseline_configs": "value = configs[2] (rs256-sd, the circuit BASELINE's metric is quoted on) on one GPU; configs[1] "
                                       "(rs256) and configs[4] (rs256-db, one replica per GPU: --gpus N) are this S21 shape with l = 20 / 28 "
                                       "instead of 26 - a few of 1.5 M wires move between the l query and gamma_abc, which no kernel's "
                                       "time can tell apart, so their rate IS `value` (all three proved at full size by tests/"
                                       "test_gpu_fullsize.py); configs[3] (mdl1 / S22 sharded over the ranks) is `sharded`, its one-GPU "
                                       "rate `shapes.mdl1`; configs[0] is the CPU path: `cpu_baseline` (those three: --full)",
                   "h_query_basis": "coefficient" if a.h_coefficient_basis else "coset evaluation (transformed at load)",
                   "proofs_per_rank": n_timed, "proofs_in_flight_per_gpu": inflight,
                   "inputs": {"host": "witness in HOST memory (pageable) -> proof through cg_prove, the metric as SURVEY 8d writes it: every "
                                      "proof uploads its %d-byte assignment first; %d assignments taken in rotation; (r,s) fresh per proof",
                              "pinned": "witness in page-locked HOST memory (cg_host_alloc) -> proof through cg_prove: every proof uploads "
                                        "its %d-byte assignment first; %d assignments taken in rotation; (r,s) fresh per proof",
                              "device": "NOT the metric as written: %d-byte assignments already resident in HBM (cg_prove_dev, --witness "
                                        "device); %d taken in rotation; (r,s) fresh per proof"}[a.witness] % (int(ws_np[0].size), len(ws_np)),
                   "witness_origin": a.witness, "caller_threads": callers,
                   "context": {"resident_GB": round(info["total_bytes"] / 1e9, 2), "tables_GB": round(info["table_bytes"] / 1e9, 2),
                               "per_slot_GB": round(info["slot_bytes"] / 1e9, 3),
                               "lone_slot_GB": round(info["lone_slot_bytes"] / 1e9, 3),     # the extra slot a proof arriving alone runs on
                               "per_slot_GB_by_kind": {k[5:-6]: round(info[k] / 1e9, 3) for k in
                                                       ("slot_entry_bytes", "slot_piece_bytes", "slot_bucket_bytes", "slot_transform_bytes",
                                                        "slot_upload_bytes")},
                               "matrices_GB": round(info["matrix_bytes"] / 1e9, 3),
                               "window_bits": info["window_bits"], "tuned": bool(info["tuned"]),
                               "retune_skipped_for_memory": info["retune_skipped_for_memory"]}},
        "latency_ms": timing.get("latency_ms"),
    }

    def g1_record(tm_):
        return {"msm_g1_pairs_per_proof": tm_["msm_g1_pairs"], "msm_g2_pairs_per_proof": tm_["msm_g2_pairs"],
                "entries_g1": tm_["entries_g1"], "entries_g2": tm_["entries_g2"],
                "g1_msm_scalar_adds_per_s": round(tm_["msm_g1_pairs"] * value, 1)}     # pairs consumed per second of whole-job time

    if not a.full:
        # a plain run ends here.  One untimed proof with the library's counters gives the G1 pairs per proof that the metric's
        # scalar-adds/s is made of (they depend on the assignment, not on the time)
        out.update(g1_record(prover.prove_dev(ws_dev[0].data_ptr(), *fresh_rs(), timings=True)[1]))
        log("steady state %.2f proofs/s (%d proofs in %.2f s; median block %.2f, spread %.1f %%); shader clock %s GHz" %
            (value, n_timed, dt, timing["median_block"]["value_this_rank"] * world, timing["median_block"]["spread_pct"],
             clock.median() if clock else None))
        emit(out)
        return

    dt_br = bracketed(prove_headline_k, a.steps, True, threads=callers)
    out["timing"]["bracketed"] = {"ms_per_step": round(dt_br / a.steps * 1e3, 3), "value": round(a.steps * world / dt_br, 3),
                                  "method": "barrier + synchronise, `steps` proofs, synchronise + barrier (max over ranks)"}
    log("steady state %.2f proofs/s (%d proofs in %.2f s; median block %.2f, spread %.1f %%); bracketed %.2f; shader clock %s GHz" %
        (value, n_timed, dt, timing["median_block"]["value_this_rank"] * world, timing["median_block"]["spread_pct"],
         a.steps * world / dt_br, clock.median() if clock else None))

    tm, phases = phase_record(prover, ws_dev[0])
    g1_pairs, g2_pairs = tm["msm_g1_pairs"], tm["msm_g2_pairs"]
    launches = max(1, tm["accum_g1_launches"])
    acc_ms = phases["accum_g1_ms"]
    alg_bytes = G1_PAIR_BYTES * g1_pairs                           # all four G1 MSMs' operands, each touched once
    achieved = alg_bytes / (acc_ms * 1e-3) / 1e9 if acc_ms > 0 else 0.0
    workload_key = "%s/%s/bits=%.2f%s" % (a.shape, a.profile, a.bits, "/coeff-basis" if a.h_coefficient_basis else "")
    pmc, pmc_current = committed_counters(workload_key)
    pmc = pmc or {}
    fingerprint = source_fingerprint()
    sustained = clock.median() if clock else None
    roof = {"kernel": "k_accum_affine_g1s (G1 bucket accumulation, signed 29-bit limbs)", "bound": "hbm", "achieved": round(achieved, 2),
            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
            "traffic": pmc.get("accum_affine_g1_hbm_bytes_per_launch") if pmc_current else None,
            "launches_per_proof": launches, "avg_launch_ms": round(acc_ms / launches, 4),
            "algorithmic_bytes_per_launch": int(alg_bytes / launches),
            "mixed_adds_per_s": round(tm["entries_g1"] / (acc_ms * 1e-3), 1) if acc_ms > 0 else None,
            "binds": False,
            "note": "carry-propagating integer work (no MFMA): this kernel is bound by VALU issue, not by HBM - the HBM "
                    "fraction is reported because the contract asks for it; the binding roofline is `roofline_valu`"}
    instr = pmc.get("valu_wave_instr_per_proof") if pmc_current else None
    # ---- what the vector ALU issues, measured on THIS box in THIS run (tools/ubench/valu_rates --json: shader cycles per
    # wave-instruction per SIMD of the three classes, by clock64 on the device), and how this tree's kernels split over the
    # classes (profiles/isa_class_counts.json: the disassembly of the library this process loaded, made by build()) ---------
    issue = {"cycles_per_wave_instr": dict(ISSUE_CYCLES), "measured_in_run": False,
             "source": "profiles/r05_e_valu_issue_rates.txt (committed; the in-run micro-benchmark did not run)"}
    if rank == 0 and not a.no_ubench:
        try:
            exe = os.path.join(ROOT, "tools", "ubench", "valu_rates")
            t_u = time.perf_counter()
            ub = json.loads(subprocess.run([exe, "--json"], capture_output=True, text=True, timeout=60, check=True).stdout.strip().splitlines()[-1])
            issue = {"cycles_per_wave_instr": ub["cycles_per_wave_instr"], "per_instruction": ub["per_instruction"], "measured_in_run": True,
                     "sustained_mad64": ub["sustained_mad64"], "seconds": round(time.perf_counter() - t_u, 2),
                     "source": "tools/ubench/valu_rates --json, run by this process between the headline and the secondary legs: " + ub["how"]}
        except Exception as e:
            issue["error"] = repr(e)
    cyc = issue["cycles_per_wave_instr"]
    mix, mix_src = dict(ISSUE_MIX), "round 5's hand count of the hot loops (no per-kernel counts for this tree)"
    simd_cycles_per_proof = None
    try:
        with open(os.path.join(ROOT, "profiles", "isa_class_counts.json")) as f:
            isa = json.load(f)
        by_kernel = pmc.get("valu_wave_instr_per_proof_by_kernel") if pmc_current else None
        if isa.get("csrc_sha16") == fingerprint and by_kernel:
            tot = {"mad64": 0.0, "other": 0.0, "simple32": 0.0}
            covered = 0.0
            for kname, n_instr in by_kernel.items():
                kc = isa["kernels"].get(kname)
                if not kc or not kc["valu"]:
                    continue
                covered += n_instr
                for c_ in tot:
                    tot[c_] += n_instr * kc[c_] / kc["valu"]
            if covered > 0.98 * sum(by_kernel.values()):
                mix = {c_: round(tot[c_] / covered, 4) for c_ in tot}
                mix_src = ("every kernel's static class split (profiles/isa_class_counts.json, disassembly of this library) weighted by its "
                           "SQ_INSTS_VALU per proof (profiles/pmc_counters.json); %.1f %% of the instructions covered" % (100.0 * covered / sum(by_kernel.values())))
                simd_cycles_per_proof = sum(tot[c_] * cyc[c_] for c_ in tot) * (instr / covered)
    except Exception:
        pass
    mix_cycles = sum(cyc[c_] * mix[c_] for c_ in mix)
    if simd_cycles_per_proof is None and instr:
        simd_cycles_per_proof = instr * mix_cycles
    per_gpu = value / world
    util = (simd_cycles_per_proof * per_gpu / (N_SIMD * sustained * 1e9)) if (simd_cycles_per_proof and sustained) else None
    roof_valu = {"bound": "valu", "scope": "whole proof (every kernel of the prove path)", "unit": "G wave-instr/s",
                 "peak": round(VALU_PEAK_HW / 1e9, 1), "peak_clock_ghz": PEAK_CLOCK_GHZ,
                 "peak_is": "256 CU x 4 SIMD x 2.4 GHz / 2 cycles per wave64 VALU instruction (SIMD-32: guides/MI355X_MICROARCH.md)",
                 "achieved": round(instr * per_gpu / 1e9, 1) if instr else None,
                 # THE fraction: SIMD issue cycles this workload needs per second / SIMD cycles the chip delivers at the clock it held
                 "frac": round(util, 4) if util else None,
                 "frac_is": "SIMD-cycle utilisation: sum over instruction classes of (wave-instructions per proof x cycles the SIMD takes to "
                            "issue one, measured in this run) x proofs/s / (1024 SIMDs x sustained shader clock)",
                 "frac_of_instruction_peak": round(instr * per_gpu / VALU_PEAK_HW, 4) if instr else None,
                 "sustained_clock_ghz": sustained,
                 "wave_instr_per_proof": instr,
                 "simd_cycles_per_proof": round(simd_cycles_per_proof) if simd_cycles_per_proof else None,
                 "issue_model": dict(issue, class_mix=mix, class_mix_source=mix_src, cycles_per_wave_instr_of_this_mix=round(mix_cycles, 3)),
                 # What the chip SUSTAINS on this arithmetic: it is power-limited.  ~60 ms of nothing but multiply-adds on every SIMD
                 # runs at the rate and clock below (in-run micro-benchmark) - well under the clock the proofs hold, because their
                 # mix is lighter.  The proofs' SIMD cycles per second, expressed in multiply-adds, against that sustained rate:
                 "power_limit": ({"sustained_mad64_G_per_s": issue["sustained_mad64"]["G_wave_instr_per_s"],
                                  "clock_ghz_under_that_load": issue["sustained_mad64"]["clock_ghz"],
                                  "achieved_in_mad64_equivalents_G_per_s": round(simd_cycles_per_proof * per_gpu / cyc["mad64"] / 1e9, 1),
                                  "frac_of_sustained_rate": round(simd_cycles_per_proof * per_gpu / cyc["mad64"] / 1e9 / issue["sustained_mad64"]["G_wave_instr_per_s"], 4),
                                  "note": "a proof's SIMD issue cycles / cycles per multiply-add = the multiply-adds that would keep the SIMDs as "
                                          "busy; over the multiply-add rate the chip holds for 60 ms at its power limit"}
                                 if simd_cycles_per_proof and issue.get("sustained_mad64") else None),
                 "legacy_frac_4_cycle_convention": round(instr * per_gpu / VALU_PEAK, 4) if instr else None,
                 "legacy_frac_of_sustained_clock_peak": round(instr * per_gpu / (VALU_PEAK * sustained / PEAK_CLOCK_GHZ), 4)
                 if instr and sustained else None,
                 "counters": {"source": "committed pass (profiles/pmc_counters.json), not this run", "csrc_sha16_of_pass": pmc.get("csrc_sha16"),
                              "csrc_sha16_of_this_tree": fingerprint, "current": bool(pmc_current)},
                 "note": "SQ_INSTS_VALU per steady-state proof from the committed rocprofv3 --pmc pass of this command for this "
                         "workload (null when none is committed for the kernel sources on disk) x this run's proofs/s per GPU; "
                         "sustained_clock_ghz is measured on the device during the timed proofs (cg_probe_shader_clock)"}
    # ---- the transforms: the one kernel family SURVEY 8d called bandwidth-sensitive (64 B per element per transform) -----------
    roof_ntt = None
    if rank == 0 and not a.headline_only:        # (profiling runs: the unit transforms would be counted into the proofs' kernels)
        try:
            logd = prover.domain_size.bit_length() - 1
            nt_ = cc.NttContext(logd, device=local_rank)
            buf_ = torch.zeros(32 << logd, dtype=torch.uint8, device=dev)
            for inv_ in (False, True):
                nt_.run_dev(buf_.data_ptr(), inverse=inv_)
            ms_ = [nt_.run_dev(buf_.data_ptr(), inverse=bool(i & 1), coset=bool(i & 2)) for i in range(8)]
            nt_.close()
            del buf_
            t_ms = sum(ms_) / len(ms_)
            alg = 64.0 * (1 << logd)
            roof_ntt = {"kernel": "k_ntt29_pass (radix-2 transform over Fr, 2^%d elements: cg_ntt_run, the kernels cg_prove's witness map runs)" % logd,
                        "bound": "hbm", "achieved": round(alg / (t_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(alg / (t_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "avg_transform_ms": round(t_ms, 4),
                        "algorithmic_bytes_per_transform": int(alg),
                        "traffic": round(pmc["ntt_first_pass_hbm_kb_per_launch_corrected"] * 1024) if pmc_current and pmc.get("ntt_first_pass_hbm_kb_per_launch_corrected") else None,
                        "traffic_is": "HBM bytes of ONE first pass (k_ntt29_pass<0,0,*>) from the committed counter pass, corrected on its own known byte count; a transform is two passes at this size",
                        "binds": False,
                        "note": "a butterfly is ~306 instructions around a 207-instruction product: the passes are bound by VALU issue "
                                "(69-76 % of their own instruction floor stand-alone), not by the 64 B per element they move; SURVEY 8d's "
                                "30 % target assumed a bandwidth-bound kernel.  Timed: eight transforms (forward / inverse, plain / coset) of the "
                                "unit entry point, canonical in and out, HIP events inside the call"}
        except Exception as e:
            roof_ntt = {"error": repr(e)}

    out.update({"roofline": roof, "roofline_valu": roof_valu, "roofline_ntt": roof_ntt, "phase_ms": phases,
                "phase_ms_note": "one proof ALONE on this throughput context, whose proofs run their kernels back to back on one stream "
                                 "each (the overlap comes from the other proofs in flight); a latency context (proof_slots = 1) spreads a "
                                 "proof over five streams: 6.3 ms (profiles/r03_l_shard_latency.txt)"})
    out.update(g1_record(tm))

    legs_s = {}                 # wall seconds of every leg after the headline (a --full run has to finish within minutes)
    out["legs_s"] = legs_s
    t_leg = [time.perf_counter()]

    def leg_done(name):
        now_ = time.perf_counter()
        legs_s[name] = round(now_ - t_leg[0], 1)
        t_leg[0] = now_

    # ---- checker, first part (rank 0, any N): the reference's acceptance criterion on a proof of the TIMED stream --------
    # (the oracle is the checker here, never the thing measured; ~1.5 s of Python pairing)
    oracle_mods = None
    if rank == 0 and not a.no_check:
        try:
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import bn254_oracle
            import cpu_ref
            import keycheck
            oracle_mods = (bn254_oracle, cpu_ref, keycheck)
            k_, r_, s_, data_ = checked_proof
            out["proof_verifies"] = bool(keycheck.verify(bn254_oracle, pk, l, w_np, data_))
            out["proof_checked"] = {"which": "proof %d of the timed stream (the latest one on the satisfying assignment)" % k_,
                                    "how": "verifier.rs:44-65 by the Python oracle's pairing on the GPU-made vk; a flipped public "
                                           "input is refused"}
            log("timed proof %d verifies: %s" % (k_, out["proof_verifies"]))
        except Exception as e:   # a checker that cannot run is reported, a proof that does not verify fails the run below
            out["proof_verifies"] = None
            out["proof_checked"] = {"error": repr(e)}
        assert out["proof_verifies"] is not False, "a proof of the timed stream does not verify"
    leg_done("proof_check")

    # N > 1: the secondary legs below run collectives on a path that no multi-GPU box has exercised before the driver's own
    # run.  Should one of them stall (a rank that failed alone leaves the others in a barrier), the headline measured above
    # must not be lost with it: after --leg-timeout seconds rank 0 prints the line as it stands here, marked `incomplete`,
    # and leaves with exit code 0; every other rank leaves five seconds later with exit code 4, so the launcher - and this
    # script when it started the ranks itself - returns non-zero: the exit status tells the truth about a run that did not
    # complete, and the line was on stdout before any rank failed.  (--strict-exit: rank 0 exits 4 too.)
    watchdog = None
    if world > 1 and a.leg_timeout > 0:
        core_line = json.dumps(out)

        def bail():
            if rank == 0:
                note = "secondary legs did not finish within %d s: line printed by the watchdog without them" % a.leg_timeout
                os.write(stdout_fd, (core_line[:-1] + ', "incomplete": %s}\n' % json.dumps(note)).encode())
            print("[bench] rank %d: watchdog after %d s in the secondary legs" % (rank, a.leg_timeout), file=sys.stderr, flush=True)
            os._exit(4 if (a.strict_exit or rank != 0) else 0)
        watchdog = threading.Timer(a.leg_timeout + (0 if rank == 0 else 5), bail)
        watchdog.daemon = True
        watchdog.start()

    # ---- the witness's origin, the other two ways: page-locked host memory, and already resident in HBM ------------------
    # (`value` above is the --witness origin, pageable host memory by default = SURVEY §8d's metric as written)
    rates = {a.witness: value}
    if not a.no_host_witness:
        hw = {"note": "the same steady-state measurement with the assignments arriving from the other origins: `value` is the "
                      "'%s' one.  From host memory every proof uploads its 32·M-byte assignment first (the reference's caller has "
                      "the witness on the host, creds/src/lib.rs:274-283); uploads overlap the other proofs in flight (proof_slots + 2 "
                      "caller threads)" % a.witness}
        hblocks = max(3, math.ceil(1500 / max(1, a.steps)) // 2)     # blocks of --steps proofs: >= 750 whatever --steps is
        hn = hblocks * a.steps
        try:
            for origin in ("host", "pinned", "device"):
                if origin == a.witness:
                    continue
                pk_ = stream_of(origin)
                thr = callers_of(origin)
                steady_stream(pk_, inflight, thr)
                d_o, rec_o, _ = measure(pk_, hn, min(a.warmup, inflight), hblocks, True, threads=thr)
                rates[origin] = hn * world / d_o
                rec = dict(rec_o, proofs_per_s=round(rates[origin], 3), ms_per_step=round(d_o / hn * 1e3, 4), over_value=round(rates[origin] / value, 4))
                if origin == "device":
                    out["timing"]["device_resident"] = dict(rec, note="assignments already in HBM (cg_prove_dev): rounds 1-4's headline")
                else:
                    hw["pageable" if origin == "host" else "pinned"] = rec
            _, tmu = prover.prove_host_ptr(pinned_buffers()[0].ptr, *fresh_rs(), timings=True)
            hw["upload_ms_one_proof_alone"] = round(tmu["upload_ms"], 3)
            hw["upload_bytes"] = int(ws_np[0].size)
            # the bytes do not depend on where the witness came from
            r_, s_ = fresh_rs()
            want_ = prover.prove_dev(ws_dev[0].data_ptr(), r_, s_).data
            same = prover.prove_host_ptr(pinned[0].ptr, r_, s_).data == want_ and prover.prove_host_ptr(ws_np[0].ctypes.data, r_, s_).data == want_
            hw["bytes_identical_to_device_resident"] = bool(same)
            assert same, "host-witness and device-resident proofs differ"
        except AssertionError:
            raise
        except Exception as e:
            hw["error"] = repr(e)
        out["host_witness"] = hw
    for hb in pinned:
        hb.close()
    del pinned[:]
    # the two-number summary the driver's parsed record keeps (it keeps `config`)
    out["config"]["host_witness"] = {"pageable_proofs_per_s": round(rates["host"], 3) if "host" in rates else None,
                                     "pinned_proofs_per_s": round(rates["pinned"], 3) if "pinned" in rates else None,
                                     "device_resident_proofs_per_s": round(rates["device"], 3) if "device" in rates else None,
                                     "value_is": a.witness}

    leg_done("host_witness")

    # ---- rate and latency against the number of proofs in flight: what a host sizing `proof_slots` for a latency budget needs
    # (the reference's server runs one task per credential and a user waits for ONE proof: sample/client_helper/src/main.rs:177-216)
    if world == 1 and not a.no_latency_curve:
        try:
            curve = []
            pk_ = stream_of(a.witness)
            for k in (1, 2, 4, 8, 16):
                if k > inflight:
                    break
                n_ = 200
                lat = []
                # n_ completions between two instants at which the pipeline is FULL: the first k completions are the ramp and
                # the last k the drain (a window that ends with the last completion counts work done before it began: +k/2n_,
                # 4 % at sixteen in flight)
                done_ = steady_stream(pk_, n_ + 2 * k, k, lat)
                rate_ = n_ / (done_[n_ + k - 1] - done_[k - 1])
                curve.append({"in_flight": k, "proofs": n_, "proofs_per_s": round(rate_, 2),
                              "latency_ms": percentiles_ms([d for t_, d in lat if done_[k - 1] < t_ <= done_[n_ + k - 1]])})
            knee = next((c_["in_flight"] for c_ in curve if c_["proofs_per_s"] >= 0.95 * max(x["proofs_per_s"] for x in curve)), None)
            out["inflight_curve"] = {"points": curve, "callers": "k host threads on the headline context (%d slots, throughput arrangement, + the lone slot a "
                                     "proof that finds nothing in flight runs on: the k = 1 point), witness from %s memory" % (inflight, a.witness),
                                     "in_flight_for_95_pct_of_the_best_rate": knee}
        except Exception as e:
            out["inflight_curve"] = {"error": repr(e)}
        leg_done("inflight_curve")

    # ---- the reference's own call, cold: files -> client_state.bin in a fresh process (creds/src/lib.rs:255-301) -------------
    if rank == 0 and world == 1 and not a.no_cold_start:
        try:
            out["cold_start"] = cold_start_record(cc, a, pk, cm, w_np, l, m, M, fresh_rs, prover, ws_dev, log)
        except AssertionError:
            raise
        except Exception as e:
            out["cold_start"] = {"error": repr(e)}
        leg_done("cold_start")

    # ---- N > 1: proofs sharded over the ranks (config 4), measured in the same run -------------------------------------
    if world > 1 and not a.no_sharded:
        if rank == a.stall_rank:
            time.sleep(10 ** 6)
        sh = {"ranks": world, "ranks_per_gpu": ranks_per_gpu, "backend_requested": a.backend}
        try:
            # the DATA plane: RCCL, opened here and nowhere else, with a deadline; every rank ends up on the same backend
            grp, used, rccl_err = open_data_group(dev, a.backend, a.rccl_deadline)
            sh["backend"] = used
            from crescent_credentials_amd import distributed as _d
            if _d.RCCL_TAINTED:      # a helper thread is still inside RCCL on this rank: what follows shares the process with it
                sh["rccl_tainted"] = _d.RCCL_TAINTED
            if rccl_err:
                sh["error"] = "%s group did not come up on this rank set: %s" % (a.backend, rccl_err)
                sh["backend_fallback"] = used
                log("sharded leg: %s -> falling back to %s" % (sh["error"], used))
            srng = random.Random(99)                     # the same (r, s) on every rank

            def whose_record_differs(sp_, w_ptr, r_):
                """after a sharded proof that differs from the unsharded context's (on every rank: they assembled the same records):
                every rank recomputes ITS OWN 384-byte record on a plain shard context (cg_prove_partial) and says which of the
                five points in the gathered record differ; then the same sharded proof is made AGAIN - a second wrong answer with
                the same points means the context's tables are wrong (load time), a right one that this proof's run was"""
                try:
                    chk = cc.Prover(pk_s, cm_s, device=local_rank, window_bits=a.window, shard_rank=rank, shard_count=world)
                    want_ = chk.prove_partial(w_ptr, r_, on_device=True)
                    chk.close()
                    got_ = bytes(sp_.last_parts)[384 * rank:384 * (rank + 1)] if sp_.last_parts is not None else b""
                    sp_.prove_dev(w_ptr, r_, 12345)                       # collective: every rank is here
                    again_ = bytes(sp_.last_parts)[384 * rank:384 * (rank + 1)]
                    names_, o_, bad_ = ("h", "l", "a", "b1", "b2"), 0, []
                    for nm_, sz_ in zip(names_, (64, 64, 64, 64, 128)):
                        if got_[o_:o_ + sz_] != want_[o_:o_ + sz_]:
                            bad_.append(nm_)
                        o_ += sz_
                    return "rank %d: %s; made again: %s" % (rank, ("points " + ", ".join(bad_) + " of its record differ") if bad_ else
                                                             "its own record is right", "the same record" if again_ == got_ else
                                                             "the right record" if again_ == want_ else "a third record")
                except Exception as e_:      # noqa: BLE001 - a diagnosis, never the failure itself
                    return "rank %d: no diagnosis (%r)" % (rank, e_)
            # The sharded proofs are made on config 4's own circuit - mdl1, S22 (BASELINE.json configs[3]: "mdl1 ... MSM sharded
            # across 8 x MI355X") - unless the run was given a shape; `value` above stays the replica rate of the headline shape.
            # (configs[4]'s shape, rs256-db, is the headline's with l = 28 instead of 26: two more of 1.5 M wires move from the l
            # query to gamma_abc, which no kernel's time can tell apart - its replica rate IS `value`; `config.baseline_configs`.)
            if a.sharded_shape != a.shape:
                ls_, ms_, Ms_ = wl.SHAPES[a.sharded_shape]
                t_w = time.time()
                cm_s, w_s_np, pk_s = make_workload(a.bits, 5, (ls_, ms_, Ms_))
                ws_s = [torch.from_numpy(x).to(dev) for x in permuted_assignments(w_s_np, ls_, 2, 9)]
                ref_s = cc.Prover(pk_s, cm_s, device=local_rank, window_bits=a.window, h_coefficient_basis=a.h_coefficient_basis)
                log("sharded leg: %s workload made and loaded in %.1fs" % (a.sharded_shape, time.time() - t_w))
            else:
                ls_, ms_, Ms_ = l, m, M
                cm_s, pk_s, ws_s, ref_s = cm, pk, ws_dev, prover
            same_shape = a.sharded_shape == a.shape
            sh["config"] = {"workload": "%s shape: D=2^%d, m=%d, M=%d, l=%d, nnz=%d (%s mix); bit_fraction=%.2f" %
                            (a.sharded_shape, ref_s.domain_size.bit_length() - 1, ms_, Ms_, ls_, cm_s.a.nnz + cm_s.b.nnz + cm_s.c.nnz, a.profile, a.bits),
                            "is": "BASELINE.json configs[3] (mdl1 sharded over the ranks)" if a.sharded_shape == "mdl1" else "the shape given with --shape / --sharded-shape"}
            kfl = max(1, a.sharded_inflight)
            # one proof at a time: a latency context (five streams); several in flight: a throughput context with kfl slots
            sp_ctx = cc.Prover(pk_s, cm_s, device=local_rank, window_bits=a.window, shard_rank=rank, shard_count=world,
                               h_coefficient_basis=a.h_coefficient_basis)
            sp = ShardedProver(sp_ctx, dev, group=grp)
            for _ in range(3):
                sp.prove_dev(ws_s[0].data_ptr(), srng.randrange(R), srng.randrange(R))
            barrier_sync(world)
            gathers0 = sp.all_gathers
            sp.reset_breakdown()
            t_start = time.perf_counter()
            for k in range(a.sharded_steps):
                sp.prove_dev(ws_s[k % len(ws_s)].data_ptr(), srng.randrange(R), srng.randrange(R))
            torch.cuda.synchronize()
            barrier_sync(world)
            ds = max_over_ranks(time.perf_counter() - t_start, world)
            gathers = sp.all_gathers - gathers0
            breakdown = sp.breakdown_ms()
            # this rank's shard with nothing else on the GPU queue (ranks that share a GPU take turns): the time a rank of a
            # real N-GPU run spends on its partial sums
            alone = None
            for turn in range(world):
                barrier_sync(world)
                if turn == rank:
                    t1 = time.perf_counter()
                    for k in range(5):
                        sp_ctx.prove_partial(ws_s[k % len(ws_s)].data_ptr(), srng.randrange(R), on_device=True)
                    alone = (time.perf_counter() - t1) / 5 * 1e3
            barrier_sync(world)
            alone_max = max_over_ranks(alone, world)
            # every rank assembled the same bytes as the unsharded context does
            r_, s_ = srng.randrange(R), srng.randrange(R)
            want = ref_s.prove_dev(ws_s[0].data_ptr(), r_, s_).data
            same = sp.prove_dev(ws_s[0].data_ptr(), r_, s_).data == want
            sh.update({"mode": "l/a/b queries range-sharded over the ranks, the h query by coset points j = rank (mod ranks) (two of a "
                               "shard's four transforms shrink by the rank count); 5 partial points per rank and proof",
                       "proofs": a.sharded_steps, "proofs_in_flight": 1,
                       "ms_per_proof": round(ds / a.sharded_steps * 1e3, 3), "proofs_per_s": round(a.sharded_steps / ds, 3),
                       "ms_breakdown_rank0": breakdown, "ms_per_shard_alone_on_its_gpu_max": round(alone_max, 3),
                       "all_gathers": gathers, "all_gather_bytes_per_rank": 384,
                       "scaling": "strong", "bytes_identical_to_unsharded": bool(same)})
            assert same, "sharded and unsharded proofs differ"
            sp_ctx.close()
            # SURVEY 8e asks for both arrangements to be measured: above every rank recomputes the witness map for its own
            # h points; here rank 0 runs it once for all shards (cg_witness_map_coset), a scatter over the data plane hands out
            # the D/N-element slices, and the ranks prove with them (cg_prove_partial_q; ranks != 0 hold no witness-map memory)
            if not a.h_coefficient_basis:
                try:
                    sc_ctx = cc.Prover(pk_s, cm_s, device=local_rank, window_bits=a.window, shard_rank=rank, shard_count=world,
                                       h_scalars_external=(rank != 0))
                    sps = ShardedProver(sc_ctx, dev, group=grp, arrangement="scatter")
                    for _ in range(3):
                        sps.prove_dev(ws_s[0].data_ptr(), srng.randrange(R), srng.randrange(R))
                    barrier_sync(world)
                    sps.reset_breakdown()
                    c0 = (sps.scatters, sps.all_gathers)
                    t_start = time.perf_counter()
                    for k in range(a.sharded_steps):
                        sps.prove_dev(ws_s[k % len(ws_s)].data_ptr(), srng.randrange(R), srng.randrange(R))
                    torch.cuda.synchronize()
                    barrier_sync(world)
                    dsc = max_over_ranks(time.perf_counter() - t_start, world)
                    r_, s_ = srng.randrange(R), srng.randrange(R)
                    same_s = sps.prove_dev(ws_s[0].data_ptr(), r_, s_).data == ref_s.prove_dev(ws_s[0].data_ptr(), r_, s_).data
                    sh["arrangements"] = {
                        "recompute": {"ms_per_proof": sh["ms_per_proof"], "collectives_per_proof": 1,
                                      "what": "every rank runs the witness map for its own h points (two full-size + two 1/N-size transforms)"},
                        "scatter": {"ms_per_proof": round(dsc / a.sharded_steps * 1e3, 3), "collectives_per_proof": 2,
                                    "scatter_bytes_per_peer": int(ref_s.domain_size * 32 // world),
                                    "scatters": sps.scatters - 1 - c0[0], "all_gathers": sps.all_gathers - 1 - c0[1],
                                    "ms_breakdown_rank0": sps.breakdown_ms(), "bytes_identical_to_unsharded": bool(same_s),
                                    "what": "rank 0 runs the witness map once (four full-size transforms), scatters the coset values, "
                                            "every rank proves with its slice"}}
                    assert same_s, "the scatter arrangement's proof differs from the unsharded one; " + whose_record_differs(sps, ws_s[0].data_ptr(), r_)
                    # the same arrangement in two calls: every rank opens the proof (its l, a, b1, b2 sums run), THEN the witness map
                    # and the scatter, then the h share - the assignment-driven MSMs leave the critical path
                    spt = ShardedProver(sc_ctx, dev, group=grp, arrangement="scatter", two_call=True)
                    for _ in range(3):
                        spt.prove_dev(ws_s[0].data_ptr(), srng.randrange(R), srng.randrange(R))
                    barrier_sync(world)
                    spt.reset_breakdown()
                    t_start = time.perf_counter()
                    for k in range(a.sharded_steps):
                        spt.prove_dev(ws_s[k % len(ws_s)].data_ptr(), srng.randrange(R), srng.randrange(R))
                    torch.cuda.synchronize()
                    barrier_sync(world)
                    dst_ = max_over_ranks(time.perf_counter() - t_start, world)
                    r_, s_ = srng.randrange(R), srng.randrange(R)
                    same_t = spt.prove_dev(ws_s[0].data_ptr(), r_, s_).data == ref_s.prove_dev(ws_s[0].data_ptr(), r_, s_).data
                    sh["arrangements"]["scatter_two_call"] = {
                        "ms_per_proof": round(dst_ / a.sharded_steps * 1e3, 3), "collectives_per_proof": 2,
                        "ms_breakdown_rank0": spt.breakdown_ms(), "bytes_identical_to_unsharded": bool(same_t),
                        "what": "cg_prove_partial_q_begin on every rank (l, a, b1, b2 partial sums queued), rank 0's witness map on its open "
                                "proof, the scatter, cg_prove_partial_q_finish with the slice (the h share)"}
                    assert same_t, "the two-call scatter arrangement's proof differs from the unsharded one; " + whose_record_differs(spt, ws_s[0].data_ptr(), r_)
                    sc_ctx.close()
                    # ... and with the witness map in two halves: rank 0 computes the a side, rank 1 the b side at the same time, each
                    # scatters its own, every shard multiplies its two slices and adds the h share (ranks 0 and 1 hold witness-map memory)
                    if world >= 2:
                        sh_ctx = cc.Prover(pk_s, cm_s, device=local_rank, window_bits=a.window, shard_rank=rank, shard_count=world,
                                           h_scalars_external=(rank > 1))
                        sph = ShardedProver(sh_ctx, dev, group=grp, arrangement="scatter", two_call=True, split_map=True)
                        for _ in range(3):
                            sph.prove_dev(ws_s[0].data_ptr(), srng.randrange(R), srng.randrange(R))
                        barrier_sync(world)
                        sph.reset_breakdown()
                        t_start = time.perf_counter()
                        for k in range(a.sharded_steps):
                            sph.prove_dev(ws_s[k % len(ws_s)].data_ptr(), srng.randrange(R), srng.randrange(R))
                        torch.cuda.synchronize()
                        barrier_sync(world)
                        dsh_ = max_over_ranks(time.perf_counter() - t_start, world)
                        r_, s_ = srng.randrange(R), srng.randrange(R)
                        same_h = sph.prove_dev(ws_s[0].data_ptr(), r_, s_).data == ref_s.prove_dev(ws_s[0].data_ptr(), r_, s_).data
                        sh["arrangements"]["scatter_two_halves"] = {
                            "ms_per_proof": round(dsh_ / a.sharded_steps * 1e3, 3), "collectives_per_proof": 3,
                            "ms_breakdown_rank0": sph.breakdown_ms(), "bytes_identical_to_unsharded": bool(same_h),
                            "what": "cg_prove_partial_q_begin everywhere; rank 0 computes vinv·a on the coset, rank 1 b on the coset (one sparse "
                                    "product + two transforms each, at the same time); two scatters; cg_prove_partial_q_finish2 multiplies the "
                                    "slices and adds the h share"}
                        assert same_h, "the two-halves scatter arrangement's proof differs from the unsharded one; " + whose_record_differs(sph, ws_s[0].data_ptr(), r_)
                        sh_ctx.close()
                    # ... and with UNEQUAL shares (cg_options.shard_span): the two ranks that compute a half carry 0.6 of an equal
                    # share of the MSMs, the other ranks the rest (tools/probe_latency.py: 1.9 against 2.2 ms by the pieces at S21 / 8)
                    if world > 2:
                        w_src = 10000.0 / world * 0.6
                        w_oth = (10000.0 - 2 * w_src) / (world - 2)
                        cuts = [0, int(w_src), int(2 * w_src)] + [int(2 * w_src + w_oth * k) for k in range(1, world - 2)] + [10000]
                        spans = [(cuts[k], cuts[k + 1]) for k in range(world)]
                        su_ctx = cc.Prover(pk_s, cm_s, device=local_rank, window_bits=a.window, shard_rank=rank, shard_count=world,
                                           shard_span=spans[rank], h_scalars_external=(rank > 1))
                        spu = ShardedProver(su_ctx, dev, group=grp, arrangement="scatter", two_call=True, split_map=True, spans=spans)
                        for _ in range(3):
                            spu.prove_dev(ws_s[0].data_ptr(), srng.randrange(R), srng.randrange(R))
                        barrier_sync(world)
                        spu.reset_breakdown()
                        t_start = time.perf_counter()
                        for k in range(a.sharded_steps):
                            spu.prove_dev(ws_s[k % len(ws_s)].data_ptr(), srng.randrange(R), srng.randrange(R))
                        torch.cuda.synchronize()
                        barrier_sync(world)
                        dsu_ = max_over_ranks(time.perf_counter() - t_start, world)
                        r_, s_ = srng.randrange(R), srng.randrange(R)
                        same_u = spu.prove_dev(ws_s[0].data_ptr(), r_, s_).data == ref_s.prove_dev(ws_s[0].data_ptr(), r_, s_).data
                        sh["arrangements"]["scatter_two_halves_unequal_shares"] = {
                            "ms_per_proof": round(dsu_ / a.sharded_steps * 1e3, 3), "collectives_per_proof": 3, "spans_per_10000": spans,
                            "ms_breakdown_rank0": spu.breakdown_ms(), "bytes_identical_to_unsharded": bool(same_u),
                            "what": "the two-halves arrangement with the two source ranks carrying 0.6 of an equal share of every query"}
                        assert same_u, "the unequal-shares arrangement's proof differs from the unsharded one (rank %d)" % rank
                        su_ctx.close()
                except AssertionError:
                    raise
                except Exception as e:
                    sh["arrangements"] = {"error": repr(e)}
            # several sharded proofs in flight per rank (the reference's host runs one task per credential concurrently,
            # sample/client_helper/src/main.rs:177-216): partial sums of proofs k+1.. on the GPU while proof k's record is
            # exchanged and finished
            if kfl > 1:
                pp_ctx = cc.Prover(pk_s, cm_s, device=local_rank, window_bits=a.window, shard_rank=rank, shard_count=world,
                                   proof_slots=kfl, h_coefficient_basis=a.h_coefficient_basis)
                pp = ShardedProver(pp_ctx, dev, group=grp)
                njobs = max(4 * kfl, a.sharded_stream)
                mk = lambda n_: [(ws_s[k % len(ws_s)].data_ptr(), srng.randrange(R), srng.randrange(R)) for k in range(n_)]
                pp.prove_stream(mk(2 * kfl), kfl)              # first proofs + the one-time re-tune
                barrier_sync(world)
                jobs = mk(njobs)
                times = []
                g0 = pp.all_gathers
                pp.reset_breakdown()
                proofs = pp.prove_stream(jobs, kfl, done_times=times)
                torch.cuda.synchronize()
                barrier_sync(world)
                times.sort()
                skip = kfl                                     # the ramp-up: the first kfl completions
                win = max_over_ranks(times[-1] - times[skip - 1], world)
                rate = (njobs - skip) / win
                same_p = proofs[0] is not None and proofs[0].data == ref_s.prove_dev(jobs[0][0], jobs[0][1], jobs[0][2]).data
                sh["in_flight"] = {"proofs_in_flight": kfl, "proofs": njobs, "proofs_per_s": round(rate, 3),
                                   "ms_per_proof": round(1e3 / rate, 3), "over_replica_rate_of_the_same_ranks": round(rate / value, 4) if same_shape else None,
                                   "ms_breakdown_rank0": pp.breakdown_ms(), "all_gathers": pp.all_gathers - g0,
                                   "bytes_identical_to_unsharded": bool(same_p),
                                   "note": "every shard repeats the two sparse products and the two full-size inverse transforms of the "
                                           "witness map (DESIGN.md 6), so sharded proofs cost more GPU time in total than whole ones: "
                                           "sharding buys latency, replicas buy throughput"}
                assert same_p, "pipelined sharded proof differs from the unsharded one"
                # the same stream in the other arrangement: ONE witness map per proof, on rank k mod ranks for job k, a scatter
                # of the coset values, cg_prove_partial_q everywhere (scatters and gathers on two groups, from two threads)
                if not a.h_coefficient_basis:
                    try:
                        pps = ShardedProver(pp_ctx, dev, group=grp, arrangement="scatter", rotate=True, stream_slots=kfl)
                        pps.prove_stream(mk(2 * kfl), kfl)
                        barrier_sync(world)
                        jobs_s = mk(njobs)
                        times_s = []
                        s0_, g0_ = pps.scatters, pps.all_gathers
                        pps.reset_breakdown()
                        proofs_s = pps.prove_stream(jobs_s, kfl, done_times=times_s)
                        torch.cuda.synchronize()
                        barrier_sync(world)
                        times_s.sort()
                        win_s = max_over_ranks(times_s[-1] - times_s[skip - 1], world)
                        rate_s = (njobs - skip) / win_s
                        same_s2 = proofs_s[0] is not None and proofs_s[0].data == ref_s.prove_dev(jobs_s[0][0], jobs_s[0][1], jobs_s[0][2]).data
                        sh["in_flight"]["scatter_rotating"] = {
                            "proofs_per_s": round(rate_s, 3), "ms_per_proof": round(1e3 / rate_s, 3),
                            "over_replica_rate_of_the_same_ranks": round(rate_s / value, 4) if same_shape else None, "over_recompute_in_flight": round(rate_s / rate, 4),
                            "scatters": pps.scatters - s0_, "all_gathers": pps.all_gathers - g0_, "ms_breakdown_rank0": pps.breakdown_ms(),
                            "bytes_identical_to_unsharded": bool(same_s2),
                            "note": "one full witness map per proof on rank (job mod ranks) instead of a partial one on every rank"}
                        assert same_s2, "the rotating-scatter stream's proof differs from the unsharded one"
                    except AssertionError:
                        raise
                    except Exception as e:
                        sh["in_flight"]["scatter_rotating"] = {"error": repr(e)}
                pp_ctx.close()
            if ref_s is not prover:
                ref_s.close()
        except AssertionError:
            raise
        except Exception as e:     # the throughput value above stands on its own: report the failure instead of losing the line
            sh["error"] = (sh.get("error", "") + " | " if sh.get("error") else "") + repr(e)
        out["sharded"] = sh
        leg_done("sharded")

    # ---- N = 1 diagnostic: one proof over k sharded contexts on this one GPU, shard by shard ----------------
    if world == 1 and a.shard_sim > 1:
        k = a.shard_sim
        shards = [cc.Prover(pk, cm, device=local_rank, shard_rank=i, shard_count=k) for i in range(k)]
        r_, s_ = fresh_rs()
        for sh in shards:
            sh.prove_partial(ws_dev[0].data_ptr(), r_, on_device=True)
            sh.prove_partial(ws_dev[0].data_ptr(), r_, on_device=True)
        per = []
        for sh in shards:
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(5):
                sh.prove_partial(ws_dev[0].data_ptr(), r_, on_device=True)
            per.append((time.perf_counter() - t1) / 5 * 1e3)
        _, tm_shard = shards[k // 2].prove_partial(ws_dev[0].data_ptr(), r_, on_device=True, timings=True)
        parts = b"".join(sh.prove_partial(ws_dev[0].data_ptr(), r_, on_device=True) for sh in shards)
        same = shards[0].assemble(parts, k, r_, s_).data == prover.prove_dev(ws_dev[0].data_ptr(), r_, s_).data
        _, ph1 = phase_record(prover, ws_dev[0])
        out["shard_sim"] = {"shards": k, "ms_per_shard_alone_on_the_gpu": [round(x, 3) for x in per], "max_ms": round(max(per), 3),
                            "unsharded_single_proof_ms": ph1["total_ms"], "bytes_identical": bool(same),
                            "phase_ms_of_one_shard": {kk: round(float(vv), 3) for kk, vv in tm_shard.items() if kk.endswith("_ms")}}
        for sh in shards:
            sh.close()

    # ---- CPU baseline: the arkworks-equivalent C restatement on this box's host cores, SAME inputs -------
    # ---- checker, second part (rank 0): is the key the bench proves on a Groth16 key for this circuit? -----------------
    if rank == 0 and oracle_mods is not None:
        try:
            bn254_oracle, cpu_ref, keycheck = oracle_mods
            t_k = time.perf_counter()
            ktrap = tuple(trap)                                   # (alpha, beta, delta, tau), the order cg_setup takes
            scal = keycheck.check_key(bn254_oracle, cpu_ref, pk, cm, l, m, M, ktrap, nthreads=cpu_ref.best_threads())
            k_, r_, s_, data_ = checked_proof
            cf = keycheck.closed_form(bn254_oracle, cpu_ref, scal, ktrap, r_, s_, w_np, l) == keycheck.decode_proof(bn254_oracle, data_)
            out["key_check"] = {"ok": True, "proof_equals_trapdoor_closed_form": bool(cf), "seconds": round(time.perf_counter() - t_k, 1),
                                "how": "oracle/keycheck.py: fixed points and gamma_abc, a strided sample, and a random linear combination "
                                       "over ALL entries of the five queries against the trapdoor's scalars (r1cs_to_qap.rs:103-147, "
                                       "generator.rs:118-194 restated in oracle/cpu_ref.c) - no code shared with cg_setup"}
            assert cf, "the timed proof is not the trapdoor's closed form"
        except AssertionError as e:
            out["key_check"] = {"ok": False, "error": repr(e)}
            raise
        except Exception as e:
            out["key_check"] = {"ok": None, "error": repr(e)}
        leg_done("key_check")

    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        try:
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import cpu_ref
            cores = cpu_ref.num_procs()
            threads = cpu_ref.best_threads(cores) if hasattr(cpu_ref, "best_threads") else min(cores, 32)
            r, s = fresh_rs()
            gpu_proof = prover.prove_dev(ws_dev[0].data_ptr(), r, s).data
            t_c = time.perf_counter()
            cpu_proof, ctm = cpu_ref.prove(pk, (cm.a, cm.b, cm.c), l, m, M, w_np, r, s, nthreads=threads, timings=True)
            wall = time.perf_counter() - t_c
            same = cpu_proof == gpu_proof
            g1_s = sum(ctm.get(k, 0.0) for k in ("msm_h_s", "msm_l_s", "msm_a_s", "msm_b1_s"))
            # one thread: the a-query G1 MSM of the same proof (M - 1 pairs) - a bounded sample; a whole proof of this size on
            # one thread would take about a minute, so the whole-proof one-thread figure is taken at an eighth of the size
            t1 = time.perf_counter()
            cpu_ref.msm_g1(pk.a_query[64:], w_np[32:], nthreads=1)
            one_thread_s = time.perf_counter() - t1
            l8, m8, M8 = wl.SHAPES["rs256-sd-eighth"]
            cm8, w8 = wl.synthetic_circuit(0xC5E5CE47 + 88, l8, m8, M8, a.bits, 3, profile=a.profile)
            pk8 = cc.generate_parameters_with_qap(cm8, *trap)
            r8, s8 = fresh_rs()
            p8 = cc.Prover(pk8, cm8, device=local_rank)
            gpu8 = p8.prove(w8, r8, s8).data
            p8.close()
            cpu8, ctm8 = cpu_ref.prove(pk8, (cm8.a, cm8.b, cm8.c), l8, m8, M8, w8, r8, s8, nthreads=1, timings=True)
            same8 = cpu8 == gpu8
            out["cpu_baseline"] = {
                "value": round(1.0 / ctm["total_s"], 5), "unit": "proofs/s", "cores": threads, "host_threads_available": cores,
                "kind": "port",
                "sample": "1 full proof of the SAME workload (same key, assignment, r, s) by oracle/cpu_ref.c, the "
                          "arkworks-equivalent C restatement, on %d threads - every CPU this process may use: %d hardware threads "
                          "visible, cgroup quota %s - (Pippenger c = ln(n) + 2 with one task per window as arkworks has it, so <= 16 "
                          "threads work during an MSM; four-step radix-2 NTT and row-parallel sparse products on all threads): "
                          "%.2fs prove (+ %.2fs key decode, not counted)" %
                          (threads, cores, cpu_ref.cpu_quota(), ctm["total_s"], ctm["load_s"]),
                "proof_bytes_identical_to_gpu": bool(same),
                "phase_s": {k: round(v, 3) for k, v in ctm.items()}, "wall_s": round(wall, 2),
                "g1_msm_scalar_adds_per_s": round(g1_pairs / g1_s, 1) if g1_s > 0 else None,
                "one_thread": {"sample": "the a-query G1 MSM of the same proof (%d pairs) on 1 thread" % (M - 1),
                               "seconds": round(one_thread_s, 3), "g1_msm_scalar_adds_per_s": round((M - 1) / one_thread_s, 1),
                               "whole_proof": {"sample": "1 full proof of the same gate mix at an eighth of the size (D = 2^18, m = %d, "
                                                         "M = %d, l = %d) on 1 thread" % (m8, M8, l8),
                                               "seconds": round(ctm8["total_s"], 3), "proofs_per_s": round(1.0 / ctm8["total_s"], 5),
                                               "phase_s": {k: round(v, 3) for k, v in ctm8.items()},
                                               "proof_bytes_identical_to_gpu": bool(same8)}},
                "cpu_quota": cpu_ref.cpu_quota() if cpu_ref.cpu_quota() != float("inf") else None,
                "gpu_over_cpu": round(value / (1.0 / ctm["total_s"]), 1)}
            if isinstance(out.get("cold_start"), dict) and "cpu_chain" in out["cold_start"]:
                cch = out["cold_start"]["cpu_chain"]
                cch["key_decode_s"] = round(ctm["load_s"], 3)
                cch["groth16_prove_s"] = round(ctm["total_s"], 3)
                cch["total_s"] = round(cch["reading_r1cs_s"] + cch["reading_prover_params_s"] + ctm["load_s"] + ctm["total_s"], 3)
                cch["threads"] = threads
                out["cold_start"]["gpu_over_cpu_cold"] = round(cch["total_s"] / out["cold_start"]["total_s"], 1)
            # no published number exists for this metric (none in the tree); the only baseline there is is
            # this same-run CPU restatement, and the ratio to it is what the field carries - named for what it is
            # (`vs_baseline` stays null: BASELINE.md §1 holds no published number for this metric.  The ratio to the same-run CPU
            # restatement is `cpu_baseline.gpu_over_cpu` - a reported baseline, not a target.)
            assert same and same8, "CPU restatement and HIP path disagree on the proof bytes"
        except Exception as e:  # the baseline is a reported number, never the thing measured
            out["cpu_baseline"] = {"value": None, "unit": "proofs/s", "cores": 0, "kind": "port", "sample": "failed: %r" % (e,)}
            if isinstance(e, AssertionError):
                raise

    leg_done("cpu_baseline")

    # ---- the second shape of SURVEY 8d's table ("S21 with l = 26 AND S22 ... report both"): mdl1, D = 2^22, measured as the
    # headline is (witness in pageable host memory, sixteen proofs in flight, steady state) over >= 300 proofs ------------------
    if rank == 0 and world == 1 and not a.no_shapes and a.shape != "mdl1":
        prover.close()
        try:
            t_w = time.time()
            l2, m2, M2 = wl.SHAPES["mdl1"]
            cm2, w2, pk2 = make_workload(a.bits, 5, (l2, m2, M2))
            p2 = cc.Prover(pk2, cm2, device=local_rank, window_bits=a.window, proof_slots=inflight, h_coefficient_basis=a.h_coefficient_basis)
            ws2 = permuted_assignments(w2, l2, 2, 9)
            made_s = time.time() - t_w

            def prove2_k(k, p2=p2, ws2=ws2):
                p2.prove_host_ptr(ws2[k % len(ws2)].ctypes.data, *fresh_rs())
            prime(prove2_k)
            d2, rec2, _ = measure(prove2_k, 300, inflight, 3, False, threads=inflight + 2)
            w2d = torch.from_numpy(ws2[0]).to(dev)
            tm2, ph2 = phase_record(p2, w2d, reps=2)
            r_, s_ = fresh_rs()
            same2 = p2.prove_host_ptr(ws2[0].ctypes.data, r_, s_).data == p2.prove_dev(w2d.data_ptr(), r_, s_).data
            info2 = p2.info()
            out["shapes"] = {"mdl1": {
                "workload": "mdl1 shape: D=2^%d, m=%d, M=%d, l=%d, nnz=%d (%s mix); bit_fraction=%.2f; pk from seeded trapdoor (GPU setup)" %
                            (p2.domain_size.bit_length() - 1, m2, M2, l2, cm2.a.nnz + cm2.b.nnz + cm2.c.nnz, a.profile, a.bits),
                "proofs_per_s": round(300 / d2, 3), "ms_per_step": round(d2 / 300 * 1e3, 4), "window_proofs": rec2["window_proofs"],
                "block_spread_pct": rec2["median_block"]["spread_pct"], "latency_ms": rec2["latency_ms"],
                "witness_origin": "host (pageable): %d-byte assignments through cg_prove, 2 in rotation, (r, s) fresh per proof" % int(ws2[0].size),
                "proofs_in_flight": inflight, "msm_g1_pairs_per_proof": tm2["msm_g1_pairs"], "entries_g1": tm2["entries_g1"],
                "g1_msm_scalar_adds_per_s": round(tm2["msm_g1_pairs"] * 300 / d2, 1), "phase_ms_one_proof_alone": ph2,
                "resident_GB": round(info2["total_bytes"] / 1e9, 2), "window_bits": info2["window_bits"], "tuned": bool(info2["tuned"]),
                "host_and_device_witness_give_the_same_bytes": bool(same2), "workload_and_key_made_and_loaded_in_s": round(made_s, 1),
                "is": "SURVEY 8d config 3's second instance / config 4's circuit on one GPU"}}
            log("mdl1 (S22): %.2f proofs/s over %d proofs" % (300 / d2, rec2["window_proofs"]))
            assert same2, "mdl1: host-witness and device-resident proofs differ"
            p2.close()
            del w2d
        except AssertionError:
            raise
        except Exception as e:
            out["shapes"] = {"mdl1": {"error": repr(e)}}
        leg_done("shapes_mdl1")

    # ---- secondary: the same measurement over the share of bit wires (the headline's one assumption) --------------------
    if rank == 0 and world == 1 and not a.no_sweep:
        prover.close()
        sweep = []
        ksteps = 100                                       # 3 blocks: a 300-proof steady window per workload
        for bf in SWEEP_FRACTIONS:
            if abs(bf - a.bits) < 1e-9:
                sweep.append({"bit_fraction": bf, "wires": wires, "nnz": nnz, "proofs_per_s": round(value, 3),
                              "g1_msm_scalar_adds_per_s": round(g1_pairs * value, 1), "entries_g1": tm["entries_g1"],
                              "entries_g2": tm["entries_g2"], "note": "the headline run"})
                continue
            cm_s, w_s, pk_s = make_workload(bf, 4 + int(bf * 100))
            ps = cc.Prover(pk_s, cm_s, device=local_rank, window_bits=a.window, proof_slots=inflight,
                           h_coefficient_basis=a.h_coefficient_basis)
            wsd = [torch.from_numpy(x).to(dev) for x in permuted_assignments(w_s, l, 2, 11)]

            def prove_sweep_k(k, ps=ps, wsd=wsd):
                ps.prove_dev(wsd[k % len(wsd)].data_ptr(), *fresh_rs())
            prime(prove_sweep_k)
            d_s, rec_s, _ = measure(prove_sweep_k, 3 * ksteps, inflight, 3, False)
            tms, phs = phase_record(ps, wsd[0], reps=1)
            sweep.append({"bit_fraction": bf, "wires": wl.wire_stats(w_s), "nnz": cm_s.a.nnz + cm_s.b.nnz + cm_s.c.nnz,
                          "proofs_per_s": round(3 * ksteps / d_s, 3), "g1_msm_scalar_adds_per_s": round(tms["msm_g1_pairs"] * 3 * ksteps / d_s, 1),
                          "entries_g1": tms["entries_g1"], "entries_g2": tms["entries_g2"],
                          "accum_g1_ms": phs["accum_g1_ms"], "witness_map_ms": phs["witness_map_ms"],
                          "window_proofs": rec_s["window_proofs"], "block_spread_pct": rec_s["median_block"]["spread_pct"]})
            ps.close()
            del wsd
        out["witness_sweep"] = sweep
        u = [x for x in sweep if x["bit_fraction"] == 0.0]
        if u:
            out["g1_msm_scalar_adds_per_s_uniform_scalars"] = u[0]["g1_msm_scalar_adds_per_s"]   # SURVEY §8d's definition
        leg_done("witness_sweep")

    if watchdog:
        watchdog.cancel()
    emit(out)


if __name__ == "__main__":
    main()
