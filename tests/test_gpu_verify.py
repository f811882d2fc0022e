"""Groth16 verification on the GPU (csrc/verify.hip, cg_verify_batch): `Groth16::verify_with_processed_vk`
(forks/groth16/src/verifier.rs:25-65) for batches of proofs under one key, checked verdict by verdict against the oracle
(oracle/ark_files.py verify_with_processed_vk): golden and fresh proofs, tampered proofs and keys, synthetic keys from
chosen scalars whose accepting proofs hit every identity skip of the Miller loop, malformed proofs and inputs (one slot
each), batch sizes across the chunk and block edges, the C caller's --verify and create_client_state(verify=True)."""
import os
import random
import subprocess

import numpy as np
import pytest

import ark_files
import bn254_oracle as o
from conftest import ROOT
import verify_vectors as V

pytestmark = pytest.mark.gpu

REJECT, ACCEPT, MALFORMED = 0, 1, 2
Q, R = o.Q, o.R


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


def _pvk(cc, vk):
    return cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(vk)))


def _verdicts(cc, pvk, inputs, proofs):
    ib = b"".join(V.inputs_bytes(x) for x in inputs)
    return list(cc.Groth16.verify_batch(pvk, np.frombuffer(ib, np.uint8), np.frombuffer(b"".join(proofs), np.uint8)))


def _pk_from_oracle(cc, pk):
    g1s = lambda pts: np.frombuffer(b"".join(o.g1_packed(p) for p in pts), dtype=np.uint8).copy()
    g2s = lambda pts: np.frombuffer(b"".join(o.g2_packed(p) for p in pts), dtype=np.uint8).copy()
    v = pk["vk"]
    vk = cc.VerifyingKey(alpha_g1=g1s([v["alpha_g1"]]), beta_g2=g2s([v["beta_g2"]]), gamma_g2=g2s([v["gamma_g2"]]),
                         delta_g1=g1s([v["delta_g1"]]), delta_g2=g2s([v["delta_g2"]]), gamma_abc_g1=g1s(v["gamma_abc_g1"]))
    return cc.ProvingKey(vk=vk, beta_g1=g1s([pk["beta_g1"]]), delta_g1=g1s([pk["delta_g1"]]), a_query=g1s(pk["a_query"]),
                         b_g1_query=g1s(pk["b_g1_query"]), b_g2_query=g2s(pk["b_g2_query"]), h_query=g1s(pk["h_query"]),
                         l_query=g1s(pk["l_query"]))


def _swap_ac(p: bytes) -> bytes:
    return p[192:256] + p[64:192] + p[0:64]


@pytest.mark.parametrize("name", ["tiny", "d8", "dummy1024"])
def test_golden_and_fresh_proofs(cc, name):
    pk, mats, w, g = V.golden_vk(name)
    l = g["num_inputs"]
    xs = w[1:l]
    golden = [bytes.fromhex(c["proof"]) for c in g["proofs"]]
    # fresh proofs of the product on the same key
    cm = cc.ConstraintMatrices.from_rows(mats[0], mats[1], mats[2], l, g["num_variables"])
    prover = cc.Prover(_pk_from_oracle(cc, pk), cm)
    rng = random.Random(len(name))
    wb = np.frombuffer(V.inputs_bytes(w), np.uint8).copy()
    fresh = [prover.prove(wb, rng.randrange(R), rng.randrange(R)).data for _ in range(2)]
    prover.close()
    proofs = golden + fresh
    flipped = list(xs); flipped[0] = (flipped[0] + 1) % R
    # the same circuit under another trapdoor: a proof under another key
    t = g["trapdoor"]
    other, _ = o.generate_parameters(mats, l, g["num_constraints"], g["num_variables"], int(t["tau"], 16) + 1, int(t["alpha"], 16),
                                     int(t["beta"], 16) + 2, int(t["delta"], 16) + 3)
    with _pvk(cc, pk["vk"]) as pvk:
        assert pvk.num_inputs == l - 1
        assert _verdicts(cc, pvk, [xs] * len(proofs), proofs) == [ACCEPT] * len(proofs)
        assert _verdicts(cc, pvk, [flipped, xs], [golden[0], _swap_ac(golden[0])]) == [REJECT, REJECT]
        assert cc.Groth16.verify_with_processed_vk(pvk, xs, golden[-1])
        assert not cc.Groth16.verify_with_processed_vk(pvk, flipped, golden[-1])
    with _pvk(cc, other["vk"]) as pvk:
        assert _verdicts(cc, pvk, [xs], [golden[0]]) == [REJECT]
    # a corrupted alpha_g1_beta_g2 (still canonical) rejects everything
    pvkb = bytearray(cc.Groth16.prepare_verifying_key(V.vk_bytes(pk["vk"])))
    at = len(V.vk_bytes(pk["vk"]))
    pvkb[at] ^= 1
    with cc.PreparedVerifyingKey(bytes(pvkb)) as pvk:
        assert _verdicts(cc, pvk, [xs], [golden[0]]) == [REJECT]
    # one input too many or too few: SynthesisError::MalformedVerifyingKey
    with _pvk(cc, pk["vk"]) as pvk:
        with pytest.raises(cc.CrescentGpuError) as e:
            cc.Groth16.verify_batch(pvk, V.inputs_bytes(xs + [1]), golden[0])
        assert e.value.code == -6


def _synthetic(ell, seed):
    rng = random.Random(seed)
    alpha, beta, gamma, delta = (rng.randrange(1, R) for _ in range(4))
    ks = [rng.randrange(R) for _ in range(ell + 1)]
    xs = [rng.randrange(R) for _ in range(ell)]
    return rng, (alpha, beta, gamma, delta, ks), xs


@pytest.mark.parametrize("ell", [1, 2, 26])
def test_synthetic_keys_identity_skips(cc, ell):
    rng, sc, xs = _synthetic(ell, 100 + ell)
    alpha, beta, gamma, delta, ks = sc
    # a second key whose prepared inputs are O for xs: k_0 = -sum x_i k_i
    ks0 = [(-sum(x * k for x, k in zip(xs, ks[1:]))) % R] + ks[1:]
    sc0 = (alpha, beta, gamma, delta, ks0)
    a, b = rng.randrange(1, R), rng.randrange(1, R)
    cases = [
        (sc, V.synthetic_proof(sc, xs, a=a, b=b)),                    # all three pairs live
        (sc0, V.synthetic_proof(sc0, xs, a=a, b=b)),                  # prepared inputs = O
        (sc, V.synthetic_proof(sc, xs, a=0, b=b)),                    # A = O
        (sc, V.synthetic_proof(sc, xs, a=a, b=0)),                    # B = O
        (sc, V.synthetic_proof(sc, xs, a=a, c=0)),                    # C = O
    ]
    bad = V.synthetic_proof(sc, xs, a=a, b=b)
    bad = (bad[0], bad[1], o.G1.to_affine(o.G1.add_affine(o.G1.to_jac(bad[2]), o.G1_GEN)))
    cases.append((sc, bad))                                           # a rejecting one
    assert cases[2][1][0] is None and cases[3][1][1] is None and cases[4][1][2] is None
    pvks = {}
    for key, pr in cases:
        vk = V.synthetic_vk(key[0], key[1], key[2], key[3], key[4])
        kid = id(key)
        if kid not in pvks:
            pvks[kid] = (_pvk(cc, vk), ark_files.prepare_verifying_key(vk))
        gpu, ora = pvks[kid]
        want = ark_files.verify_with_processed_vk(ora, xs, pr)
        got = _verdicts(cc, gpu, [xs], [V.proof_bytes(pr)])[0]
        assert got == (ACCEPT if want else REJECT)
    assert [ark_files.verify_with_processed_vk(pvks[id(k)][1], xs, p) for k, p in cases] == [True] * 5 + [False]
    for gpu, _ in pvks.values():
        gpu.close()


def _malformed_cases(sc, xs, good):
    rng = random.Random(7)
    a, b, c = good
    out = []
    off = (a[0], (a[1] + 1) % Q)
    out.append(("off-curve A", xs, V.proof_bytes((off, b, c))))
    out.append(("B on the twist outside G2", xs, V.proof_bytes((a, V.twist_point_outside_g2(rng), c))))
    p = bytearray(V.proof_bytes(good)); p[192:224] = Q.to_bytes(32, "little")
    out.append(("C.x = q", xs, bytes(p)))
    p = bytearray(V.proof_bytes(good)); p[64:96] = (Q + 5).to_bytes(32, "little")
    out.append(("B.x.c0 > q", xs, bytes(p)))
    p = bytearray(V.proof_bytes(good)); p[63] |= 0xC0
    out.append(("A with both flags", xs, bytes(p)))
    p = bytearray(V.proof_bytes(good)); p[0:64] = bytes(64)
    out.append(("A = (0, 0) without the infinity flag", xs, bytes(p)))
    bad_in = list(xs); bad_in[-1] = R
    out.append(("input = r", bad_in, V.proof_bytes(good)))
    return out


def test_malformed_slots(cc):
    rng, sc, xs = _synthetic(2, 5)
    good = V.synthetic_proof(sc, xs, a=rng.randrange(1, R), b=rng.randrange(1, R))
    cases = _malformed_cases(sc, xs, good)
    inputs, proofs, want = [], [], []
    for what, x, p in cases:
        inputs += [xs, x]
        proofs += [V.proof_bytes(good), p]
        want += [ACCEPT, MALFORMED]
    with _pvk(cc, V.synthetic_vk(*sc[:4], sc[4])) as pvk:
        got = _verdicts(cc, pvk, inputs, proofs)
    assert got == want, [(c[0], g) for c, g in zip(cases, got[1::2])]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 65536])
def test_batch_sizes(cc, n):
    rng, sc, xs = _synthetic(2, 9)
    good = V.synthetic_proof(sc, xs, a=rng.randrange(1, R), b=rng.randrange(1, R))
    flipped = list(xs); flipped[1] = (flipped[1] + 1) % R
    mal = _malformed_cases(sc, xs, good)[0]
    kinds = [(xs, V.proof_bytes(good), ACCEPT), (flipped, V.proof_bytes(good), REJECT), (mal[1], mal[2], MALFORMED),
             (xs, _swap_ac(V.proof_bytes(good)), REJECT)]
    sel = np.zeros(n, np.int64)
    pick = random.Random(n)
    for pos in pick.sample(range(n), min(n, 8)):
        sel[pos] = pick.randrange(1, len(kinds))
    ib = np.stack([np.frombuffer(V.inputs_bytes(k[0]), np.uint8) for k in kinds])[sel].reshape(-1)
    pb = np.stack([np.frombuffer(k[1], np.uint8) for k in kinds])[sel].reshape(-1)
    want = np.array([k[2] for k in kinds], np.uint8)[sel]
    with _pvk(cc, V.synthetic_vk(*sc[:4], sc[4])) as pvk:
        got = cc.Groth16.verify_batch(pvk, ib, pb)
    assert got.shape == (n,)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]


@pytest.fixture(scope="module")
def files(cc):
    """a Crescent cache directory for a small synthetic circuit: main_c.r1cs, prover_params.bin (GPU setup, pvk by
    cg_prepare_verifying_key), witness"""
    from crescent_credentials_amd import workloads as wl
    l, m, M = 5, 600, 640
    cm, w = wl.synthetic_circuit(31337, l, m, M, 0.85, 3, profile="gates")
    rows = wl.matrices_to_rows(cm)
    r1cs = ark_files.r1cs_file_bytes(rows, M, 2, l - 3, M - l)
    rng = random.Random(5150)
    pk = cc.generate_parameters_with_qap(cm, *[rng.randrange(1, R) for _ in range(4)])
    n_abc = pk.vk.gamma_abc_g1.size // 64
    vk_bytes = cc.proving_key_to_bytes(pk)[:512 + 8 + 64 * n_abc]     # the VerifyingKey leads the serialized ProvingKey
    pvk = cc.Groth16.prepare_verifying_key(vk_bytes)
    pp = cc.ProverParams(pk, pvk, '{"alg": "RS256"}').to_bytes()
    at = pp.find(pvk)
    bad = bytearray(pp)
    vk_len = len(cc.ProverParams.from_bytes(pp).vk_bytes)
    bad[at + vk_len] ^= 1                                   # alpha_g1_beta_g2, still canonical
    return dict(l=l, M=M, w=w, r1cs=r1cs, pp=pp, bad_pp=bytes(bad), pvk=pvk)


def test_c_caller_verify(cc, files, tmp_path):
    exe = os.path.join(ROOT, "integration", "c", "crescent_prove")
    (tmp_path / "main_c.r1cs").write_bytes(files["r1cs"])
    (tmp_path / "pp.bin").write_bytes(files["pp"])
    (tmp_path / "bad_pp.bin").write_bytes(files["bad_pp"])
    (tmp_path / "witness.bin").write_bytes(files["w"].tobytes())
    rs = ["--rs", "1234567", "89abcdef"]
    base = [exe, str(tmp_path / "main_c.r1cs"), str(tmp_path / "pp.bin"), str(tmp_path / "witness.bin")]
    r0 = subprocess.run(base + [str(tmp_path / "cs0.bin")] + rs + ["--sync-load", "--timings-json"], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0, r0.stderr
    assert "verify_ms" not in r0.stdout
    r1 = subprocess.run(base + [str(tmp_path / "cs1.bin")] + rs + ["--sync-load", "--timings-json", "--verify"], capture_output=True,
                        text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr
    assert '"verify_ms": ' in r1.stdout
    assert (tmp_path / "cs0.bin").read_bytes() == (tmp_path / "cs1.bin").read_bytes()
    bad = [exe, str(tmp_path / "main_c.r1cs"), str(tmp_path / "bad_pp.bin"), str(tmp_path / "witness.bin"), str(tmp_path / "cs2.bin")]
    r2 = subprocess.run(bad + rs + ["--verify"], capture_output=True, text=True, timeout=300)
    assert r2.returncode != 0 and "does not verify" in r2.stderr
    assert not (tmp_path / "cs2.bin").exists()


def test_create_client_state_verify(cc, files):
    cs = cc.create_client_state(files["r1cs"], files["pp"], files["w"], random.Random(1), verify=True)
    assert cs.pvk == files["pvk"]
    with pytest.raises(cc.ProofRejected):
        cc.create_client_state(files["r1cs"], files["bad_pp"], files["w"], random.Random(1), verify=True)
