"""Test vectors for Groth16 verification (csrc/pairing.hpp, csrc/verify.hip), built with the oracle only: Fq12 / G2
helpers, twist points outside G2, synthetic keys from chosen scalars, and the golden circuits' verifying keys.  Shared by
tests/test_pairing_host.py, tests/test_verify_cpu.py and tests/test_gpu_verify.py."""
import random

import ark_files
import bn254_oracle as o
from conftest import load_golden

Q, R = o.Q, o.R
F2 = o.Fq2Ops


def fq2_pow(a, e):
    r = F2.one
    for bit in bin(e)[2:]:
        r = F2.sqr(r)
        if bit == "1":
            r = F2.mul(r, a)
    return r


def fq2_sqrt(a):
    """square root in Fq2 for q = 3 (mod 4) (Adj, Rodriguez-Henriquez, alg. 9); None when a is not a square"""
    a1 = fq2_pow(a, (Q - 3) // 4)
    alpha = F2.mul(a1, F2.mul(a1, a))
    a0 = F2.mul((alpha[0], (-alpha[1]) % Q), alpha)
    if a0 == (Q - 1, 0):
        return None
    x0 = F2.mul(a1, a)
    if alpha == (Q - 1, 0):
        x = F2.mul((0, 1), x0)
    else:
        x = F2.mul(fq2_pow(F2.add(F2.one, alpha), (Q - 1) // 2), x0)
    return x if F2.sqr(x) == a else None


def twist_point_outside_g2(rng):
    """a point on the twist y^2 = x^3 + b' whose order is not r"""
    while True:
        x = (rng.randrange(Q), rng.randrange(Q))
        y = fq2_sqrt(F2.add(F2.mul(F2.sqr(x), x), o.B2))
        if y is None:
            continue
        P = (x, y)
        if o.G2.to_affine(o.G2.mul_affine(P, R)) is not None:
            return P


def random_f12(rng):
    return [rng.randrange(Q) for _ in range(12)]


def g1(k):
    return o.G1.to_affine(o.G1.mul_affine(o.G1_GEN, k % R))


def g2(k):
    return o.G2.to_affine(o.G2.mul_affine(o.G2_GEN, k % R))


def g1_hex(P):
    return o.g1_packed(P).hex()


def g2_hex(P):
    return o.g2_packed(P).hex()


def vk_bytes(vk) -> bytes:
    return o.vk_uncompressed(vk)


def synthetic_vk(alpha, beta, gamma, delta, ks):
    """a VerifyingKey from chosen scalars: gamma_abc_g1[i] = k_i·G1"""
    return dict(alpha_g1=g1(alpha), beta_g2=g2(beta), gamma_g2=g2(gamma), delta_g1=g1(delta), delta_g2=g2(delta),
                gamma_abc_g1=[g1(k) for k in ks])


def synthetic_proof(sc, inputs, a=None, b=None, c=None):
    """(A, B, C) = (a G1, b G2, c G1) with ab = alpha beta + (k_0 + sum x_i k_i) gamma + c delta; exactly one of a, b, c
    may be left None and is solved for (a = 0, b = 0 or c = 0 give the identity)"""
    alpha, beta, gamma, delta, ks = sc
    K = (ks[0] + sum(x * k for x, k in zip(inputs, ks[1:]))) % R
    rhs0 = (alpha * beta + K * gamma) % R
    if c is None:
        c = (a * b - rhs0) * pow(delta, R - 2, R) % R
    elif b is None:
        b = (rhs0 + c * delta) * pow(a, R - 2, R) % R
    elif a is None:
        a = (rhs0 + c * delta) * pow(b, R - 2, R) % R
    assert (a * b - rhs0 - c * delta) % R == 0
    return (g1(a), g2(b), g1(c))


def proof_bytes(pr) -> bytes:
    return o.proof_uncompressed(pr)


def inputs_bytes(xs) -> bytes:
    return b"".join(int(x).to_bytes(32, "little") for x in xs)


def golden_vk(name):
    """(vk, public inputs, [(r, s, proof bytes)]) of a golden circuit; the key is regenerated from its trapdoor"""
    g = load_golden("groth16_%s.json" % name)
    t = g["trapdoor"]
    if "dummy" in g:
        d = g["dummy"]
        mats, l, m, M, w = o.dummy_circuit(int(d["a"], 16), int(d["b"], 16), d["num_variables"], d["num_constraints"], d["num_inputs"])
    else:
        mats = tuple([[(int(c, 16), col) for c, col in row] for row in mat] for mat in g["matrices"])
        l, m, M = g["num_inputs"], g["num_constraints"], g["num_variables"]
        w = [int(x, 16) for x in g["witness"]]
    pk, _ = o.generate_parameters(mats, l, m, M, int(t["tau"], 16), int(t["alpha"], 16), int(t["beta"], 16), int(t["delta"], 16))
    return pk, mats, w, g


def oracle_pvk_bytes(vk) -> bytes:
    return ark_files.pvk_bytes(ark_files.prepare_verifying_key(vk))


def rng(seed):
    return random.Random(seed)
