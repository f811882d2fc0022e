"""Assignments in arkworks' in-memory (Montgomery) form on the GPU: CG_FLAG_SCALARS_MONTGOMERY on proving contexts and MSM
handles, cg_qap_load_form on the key-less handle.

Truth: the committed golden proofs, and a context WITHOUT the flag fed the canonical bytes of the same values.  The
Montgomery bytes are made here from Python integers (x * 2**256 % r), never by the library.  The goldens have M = 7, 240
and 925 variables (below, short of and not a multiple of one 256-lane block of the conversion pass; D = 8, 256, 1024)."""
import json
import os
import random
import subprocess
import threading

import numpy as np
import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
INVALID, UNSATISFIED = -1, -8
GOLDENS = ["groth16_d8.json", "groth16_tiny.json", "groth16_dummy1024.json"]


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


def _mont(x):
    return x * 2**256 % R


def _pack(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8).copy()


def _ints(buf):
    b = bytes(buf)
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _mont_pack(vals):
    return _pack([_mont(v) for v in vals])


@pytest.fixture(scope="module")
def goldens(cc, oracle):
    """name -> the golden, its matrices (resident form and rows), key, witness as integers / canonical bytes / Montgomery bytes"""
    from test_gpu_parity import _case_matrices, _pk_from_json
    out = {}
    for name in GOLDENS:
        g = load_golden(name)
        cm, mats = _case_matrices(cc, oracle, g)
        if "pk" in g:
            pk = _pk_from_json(cc, g["pk"])
        else:
            t = g["trapdoor"]
            pk = cc.generate_parameters_with_qap(cm, int(t["alpha"], 16), int(t["beta"], 16), int(t["delta"], 16), int(t["tau"], 16))
        wi = [int(x, 16) for x in g["witness"]]
        cases = [(int(c["r"], 16), int(c["s"], 16), c["proof"]) for c in g["proofs"]]
        out[name] = dict(g=g, cm=cm, mats=mats, pk=pk, wi=wi, w=_pack(wi), wm=_mont_pack(wi), cases=cases, M=len(wi))
    return out


def _edge_assignment(M, seed):
    """an arbitrary assignment (nothing checks it against the constraints) that holds 0, 1 and r-1"""
    rng = random.Random(seed)
    vals = [1] + [rng.randrange(R) for _ in range(M - 1)]
    for at, v in zip(rng.sample(range(1, M), min(3, M - 1)), (0, 1, R - 1)):
        vals[at] = v
    return vals


# ---------------------------------------------------------------------------------------------- proof bytes
@pytest.mark.parametrize("coeff_basis", [False, True], ids=["folded", "h_coefficient_basis"])
@pytest.mark.parametrize("name", GOLDENS)
def test_proof_bytes_from_host_and_device_memory(cc, goldens, name, coeff_basis):
    import torch
    c = goldens[name]
    canon = cc.Prover(c["pk"], c["cm"], h_coefficient_basis=coeff_basis)
    mont = cc.Prover(c["pk"], c["cm"], h_coefficient_basis=coeff_basis, scalars_montgomery=True)
    locked = cc.HostBuffer(c["M"] * 32)
    try:
        locked.array[:] = c["wm"]
        d = torch.from_numpy(c["wm"].copy()).cuda()
        torch.cuda.synchronize()
        for r, s, want in c["cases"]:
            assert canon.prove(c["w"], r, s).data.hex() == want
            assert mont.prove(c["wm"], r, s).data.hex() == want, "pageable"
            assert mont.prove_host_ptr(locked.ptr, r, s).data.hex() == want, "page-locked"
            assert mont.prove_dev(d.data_ptr(), r, s).data.hex() == want, "device"
            assert bytes(d.cpu().numpy()) == bytes(c["wm"]), "the caller's device buffer was written"
        assert bytes(locked.array) == bytes(c["wm"])
        # the context takes the flag's form only: the canonical bytes of the same witness are another assignment
        r, s, want = c["cases"][-1]
        try:
            assert mont.prove(c["w"], r, s).data.hex() != want
        except cc.CrescentGpuError as e:                # (canonical bytes read as Montgomery may also be >= r)
            assert e.code == INVALID
        assert mont.prove(c["wm"], r, s).data.hex() == want
        # timings: the copy alone in upload_ms, the pass on its own and inside the total
        p, tm = mont.prove(c["wm"], r, s, timings=True)
        assert p.data.hex() == want and tm["reserved_ms"] > 0.0 and tm["total_ms"] >= tm["upload_ms"] + tm["reserved_ms"]
        p, tm = mont.prove_dev(d.data_ptr(), r, s, timings=True)
        assert p.data.hex() == want and tm["upload_ms"] == 0.0 and tm["reserved_ms"] > 0.0
        assert canon.prove(c["w"], r, s, timings=True)[1]["reserved_ms"] == 0.0
        assert mont.info()["slot_upload_bytes"] == canon.info()["slot_upload_bytes"]
    finally:
        locked.close()
        canon.close()
        mont.close()


@pytest.mark.parametrize("name", ["groth16_tiny.json", "groth16_dummy1024.json"])
def test_one_and_four_slots_lone_slots_included(cc, goldens, name):
    c = goldens[name]
    for slots in (1, 4):
        p = cc.Prover(c["pk"], c["cm"], proof_slots=slots, scalars_montgomery=True)
        try:
            if slots == 4:
                assert p.info()["lone_slots"] >= 1
            for r, s, want in c["cases"] * 2:                           # one at a time: on a lone slot where there is one
                assert p.prove(c["wm"], r, s).data.hex() == want, slots
            errors = []
            start = threading.Barrier(6)

            def run(k):
                try:
                    start.wait()
                    for it in range(3):
                        r, s, want = c["cases"][(k + it) % len(c["cases"])]
                        assert p.prove(c["wm"], r, s).data.hex() == want, (k, it)
                except BaseException as e:      # noqa: BLE001
                    errors.append((k, repr(e)))

            ts = [threading.Thread(target=run, args=(k,)) for k in range(6)]   # more callers than slots: the one-stream slots too
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            assert errors == []
        finally:
            p.close()


@pytest.mark.parametrize("name", ["groth16_tiny.json", "groth16_dummy1024.json"])
def test_staged_load_before_and_after_the_swap(cc, goldens, name):
    c = goldens[name]
    p = cc.Prover(c["pk"], c["cm"], staged_load=True, scalars_montgomery=True)
    try:
        assert p.load_timings()["staged"] == 1
        r, s, want = c["cases"][0]
        assert p.prove(c["wm"], r, s).data.hex() == want, "before wait_ready"
        assert p.wait_ready(120000)
        assert p.info()["warmup"] == 0
        for r, s, want in c["cases"]:
            assert p.prove(c["wm"], r, s).data.hex() == want, "after wait_ready"
    finally:
        p.close()


@pytest.mark.parametrize("name", GOLDENS)
def test_two_assignments_back_to_back(cc, goldens, name):
    """a stale upload buffer would prove the previous assignment"""
    c = goldens[name]
    other = _edge_assignment(c["M"], 5)
    canon = cc.Prover(c["pk"], c["cm"])
    mont = cc.Prover(c["pk"], c["cm"], scalars_montgomery=True)
    try:
        r, s, want = c["cases"][-1]
        want_other = canon.prove(_pack(other), r, s).data.hex()
        assert want_other != want
        om = _mont_pack(other)
        for _ in range(3):
            assert mont.prove(c["wm"], r, s).data.hex() == want
            assert mont.prove(om, r, s).data.hex() == want_other
    finally:
        canon.close()
        mont.close()


# ---------------------------------------------------------------------------------------------- elements that are no field elements
def _raw_prove(cc, prover, w, r, s, dev_ptr=None):
    out = np.full(256, 0xAB, np.uint8)
    rb, sb = _pack([r]), _pack([s])
    if dev_ptr is None:
        w = np.ascontiguousarray(w, np.uint8)
        rc = cc.lib().cg_prove(prover._h, w.ctypes.data, rb.ctypes.data, sb.ctypes.data, out.ctypes.data, None)
    else:
        rc = cc.lib().cg_prove_dev(prover._h, dev_ptr, rb.ctypes.data, sb.ctypes.data, out.ctypes.data, None)
    return rc, bytes(out), cc.lib().cg_last_error().decode()


@pytest.mark.parametrize("name", GOLDENS)
def test_element_not_below_r_is_refused_and_the_next_proof_is_right(cc, goldens, name):
    import torch
    c = goldens[name]
    M = c["M"]
    mont = cc.Prover(c["pk"], c["cm"], scalars_montgomery=True)
    try:
        r, s, want = c["cases"][0]
        for at in (0, M - 1):
            for bad in (R, 2**256 - 1):
                w = c["wm"].copy()
                w[32 * at:32 * at + 32] = _pack([bad])
                rc, out, msg = _raw_prove(cc, mont, w, r, s)
                assert rc == INVALID and out == b"\xab" * 256 and "modulus" in msg, (at, hex(bad), rc, msg)
                d = torch.from_numpy(w).cuda()
                torch.cuda.synchronize()
                rc, out, msg = _raw_prove(cc, mont, None, r, s, dev_ptr=d.data_ptr())
                assert rc == INVALID and out == b"\xab" * 256 and "modulus" in msg, ("device", at, hex(bad), rc, msg)
                for call in (lambda: mont.check_witness(w), lambda: mont.witness_map(w)):
                    with pytest.raises(cc.CrescentGpuError) as e:
                        call()
                    assert e.value.code == INVALID and not isinstance(e.value, cc.UnsatisfiedWitness)
                assert mont.prove(c["wm"], r, s).data.hex() == want, "the proof after the refusal"
    finally:
        mont.close()


# ---------------------------------------------------------------------------------------------- witness check
def _ev(row, wi):
    return sum(co * wi[col] for co, col in row) % R


def _truth(mats, wi):
    A, B, Cm = mats
    bad = []
    for i in range(len(A)):
        a, b, c = _ev(A[i], wi), _ev(B[i], wi), _ev(Cm[i], wi)
        if a * b % R != c:
            bad.append((i, a, b, c))
    return bad


@pytest.mark.parametrize("name", ["groth16_d8.json", "groth16_tiny.json"])
def test_witness_check_reports_canonical_values(cc, goldens, name):
    """one wire changed - the first wire from 1 on whose change breaks a row, as in test_gpu_witness_check.py: the same
    first_unsatisfied, n_unsatisfied and canonical a / b / c as the context without the flag (and as Python says)"""
    c = goldens[name]
    assert _truth(c["mats"], c["wi"]) == []
    w2, bad = None, []
    for wire in range(1, c["M"]):
        w2 = list(c["wi"])
        w2[wire] = (w2[wire] + 1) % R
        bad = _truth(c["mats"], w2)
        if bad:
            break
    assert bad
    canon = cc.Prover(c["pk"], c["cm"])
    mont = cc.Prover(c["pk"], c["cm"], scalars_montgomery=True)
    flagged = cc.Prover(c["pk"], c["cm"], scalars_montgomery=True, check_witness=True)
    try:
        want = canon.check_witness(_pack(w2))
        assert (want.n_unsatisfied, want.first_unsatisfied, want.a, want.b, want.c) == (len(bad),) + bad[0]
        for p in (mont, flagged):
            got = p.check_witness(_mont_pack(w2))
            assert (got.n_unsatisfied, got.first_unsatisfied, got.a, got.b, got.c) == (want.n_unsatisfied, want.first_unsatisfied, want.a, want.b, want.c)
            assert p.check_witness(c["wm"]).satisfied
        r, s, proof = c["cases"][0]
        rc, out, msg = _raw_prove(cc, flagged, _mont_pack(w2), r, s)
        assert rc == UNSATISFIED and out == b"\xab" * 256
        assert msg == "constraint %d of %d is not satisfied (%d in all)" % (bad[0][0], c["g"]["num_constraints"], len(bad)), msg
        with pytest.raises(cc.UnsatisfiedWitness):
            flagged.witness_map(_mont_pack(w2))
        assert flagged.prove(c["wm"], r, s).data.hex() == proof
    finally:
        canon.close()
        mont.close()
        flagged.close()


# ---------------------------------------------------------------------------------------------- witness map
@pytest.mark.parametrize("name", GOLDENS)
def test_witness_map_returns_montgomery_coefficients(cc, goldens, name):
    import hashlib
    import torch
    c = goldens[name]
    D = c["g"]["domain_size"]
    edge = _edge_assignment(c["M"], 9)
    assert {0, 1, R - 1} <= set(edge)
    canon = cc.Prover(c["pk"], c["cm"], h_coefficient_basis=True)
    mont = cc.Prover(c["pk"], c["cm"], scalars_montgomery=True)
    q0 = cc.QapContext(c["cm"])
    q1 = cc.QapContext(c["cm"], scalar_form=1)
    try:
        assert q1.domain_size == D == mont.domain_size
        for vals in (c["wi"], edge):
            h = canon.witness_map(_pack(vals))
            if vals is c["wi"]:
                assert hashlib.sha256(bytes(h)).hexdigest() == c["g"]["h_sha256"]
            want = [_mont(x) for x in _ints(h)]
            assert _ints(q0.witness_map(_pack(vals))) == _ints(h)
            wm = _mont_pack(vals)
            assert _ints(mont.witness_map(wm)) == want, "cg_witness_map"
            assert _ints(q1.witness_map(wm)) == want, "cg_qap_witness_map, host buffers"
            d_w = torch.from_numpy(wm.copy()).cuda()
            d_h = torch.zeros(D * 32, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            q1.witness_map_dev(d_w.data_ptr(), d_h.data_ptr())
            assert _ints(d_h.cpu().numpy()) == want, "cg_qap_witness_map, device buffers"
            assert bytes(d_w.cpu().numpy()) == bytes(wm), "the caller's device assignment was written"
            assert q1.check_witness(wm).satisfied == q0.check_witness(_pack(vals)).satisfied
            assert q1.check_witness(d_w.data_ptr(), on_device=True).n_unsatisfied == q0.check_witness(_pack(vals)).n_unsatisfied
        # an element >= r on the key-less handle, first and last index
        for at in (0, c["M"] - 1):
            w = c["wm"].copy()
            w[32 * at:32 * at + 32] = _pack([R])
            for call in (lambda: q1.witness_map(w), lambda: q1.check_witness(w)):
                with pytest.raises(cc.CrescentGpuError) as e:
                    call()
                assert e.value.code == INVALID and "modulus" in str(e.value)
        assert _ints(q1.witness_map(c["wm"])) == [_mont(x) for x in _ints(canon.witness_map(c["w"]))]
    finally:
        for x in (canon, mont, q0, q1):
            x.close()


# ---------------------------------------------------------------------------------------------- MSM handles
@pytest.fixture(scope="module")
def msm_case(oracle):
    from test_gpu_parity import _msm_case_bases
    case = [c for c in load_golden("msm.json")["cases"] if c["n"] == 1000][0]
    b1, b2, _ = _msm_case_bases(oracle, case)
    return case, b1, b2, [int(x, 16) for x in case["scalars"]]


@pytest.mark.parametrize("group", [1, 2])
def test_msm_handle_with_montgomery_scalars(cc, msm_case, group):
    import torch
    case, b1, b2, scalars = msm_case
    n_bases = 1000 if group == 1 else 300                  # the G2 list is shorter: 1000 scalars then exceed the bases
    bases = b1 if group == 1 else b2[:128 * n_bases]
    canon = cc.MsmContext(bases, group=group)
    mont = cc.MsmContext(bases, group=group, scalars_montgomery=True)
    try:
        if group == 1:
            assert mont.run(_mont_pack(scalars)).hex() == case["g1_result"]
        edged = [0, 1, R - 1] + scalars[3:]
        for n in (0, 1, 300, 1000):                        # n_scalars < n_bases, = and (G2) > n_bases
            for vals in (scalars[:n], edged[:n]):
                want = canon.run(_pack(vals))
                assert mont.run(_mont_pack(vals)) == want, (group, n)
                if n:
                    sm = _mont_pack(vals)
                    d = torch.from_numpy(sm.copy()).cuda()
                    torch.cuda.synchronize()
                    assert mont.run_dev(d.data_ptr(), n) == want, (group, n, "device")
                    assert bytes(d.cpu().numpy()) == bytes(sm), "the caller's device scalars were written"
        # an element >= r among the pairs the MSM uses is refused; one past them is never looked at
        used = min(300, n_bases)
        for at in (0, used - 1):
            for bad in (R, 2**256 - 1):
                sm = _mont_pack(scalars[:300])
                sm[32 * at:32 * at + 32] = _pack([bad])
                with pytest.raises(cc.CrescentGpuError) as e:
                    mont.run(sm)
                assert e.value.code == INVALID
        sm = np.concatenate([_mont_pack(scalars[:n_bases]), _pack([R])])
        assert mont.run(sm) == canon.run(_pack(scalars[:n_bases]))
    finally:
        canon.close()
        mont.close()


# ---------------------------------------------------------------------------------------------- shards
def test_two_flagged_shards_and_the_vectors_that_stay_canonical(cc, goldens):
    c = goldens["groth16_tiny.json"]
    plain = cc.Prover(c["pk"], c["cm"], shard_rank=0, shard_count=2)
    shards = [cc.Prover(c["pk"], c["cm"], shard_rank=k, shard_count=2, scalars_montgomery=True) for k in range(2)]
    try:
        for r, s, want in c["cases"]:
            parts = b"".join(p.prove_partial(c["wm"], r) for p in shards)
            assert shards[0].assemble(parts, 2, r, s).data.hex() == want
        # the coset values pass from shard to shard and no host computes with them: canonical on both kinds of context
        q = plain.witness_map_coset(c["w"])
        assert bytes(shards[0].witness_map_coset(c["wm"])) == bytes(q)
        for which in (0, 1):
            assert bytes(shards[0].witness_map_coset_half(c["wm"], which)) == bytes(plain.witness_map_coset_half(c["w"], which))
        slices = [shards[0].h_scalars_slice(k) for k in range(2)]
        for r, s, want in c["cases"]:
            parts = b"".join(p.prove_partial_q(c["wm"], q[32 * o:32 * (o + n)], r) for p, (o, n) in zip(shards, slices))
            assert shards[1].assemble(parts, 2, r, s).data.hex() == want
            # the two-call form: the frame holds the converted assignment from begin to finish
            opened = [p.prove_partial_q_begin(c["wm"], r) for p in shards]
            assert bytes(opened[0].witness_map_coset()) == bytes(q)
            parts = b"".join(op.finish(q[32 * o:32 * (o + n)]) for op, (o, n) in zip(opened, slices))
            assert shards[0].assemble(parts, 2, r, s).data.hex() == want
        # a Montgomery slice is NOT what the shards take
        o, n = slices[0]
        qm = _mont_pack(_ints(q[32 * o:32 * (o + n)]))
        r, s, want = c["cases"][-1]
        try:
            parts = shards[0].prove_partial_q(c["wm"], qm, r) + shards[1].prove_partial_q(c["wm"], q[32 * slices[1][0]:32 * sum(slices[1])], r)
            assert shards[0].assemble(parts, 2, r, s).data.hex() != want
        except cc.CrescentGpuError as e:
            assert e.code == INVALID
    finally:
        plain.close()
        for p in shards:
            p.close()


# ---------------------------------------------------------------------------------------------- the C host
def test_c_throughput_host_with_montgomery_witnesses():
    exe = os.path.join(ROOT, "integration", "c", "crescent_throughput")
    assert os.path.exists(exe), "build() did not produce integration/c/crescent_throughput"
    run = subprocess.run([exe, "--shape", "6", "3000", "3100", "--slots", "2", "--proofs", "12", "--warmup", "2", "--montgomery"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    d = json.loads(run.stdout.strip().splitlines()[-1])
    assert d["scalars"] == "montgomery" and d["proofs"] == 12 and d["proof_slots"] == 2 and d["host_scalars_convert_ms"] > 0.0
