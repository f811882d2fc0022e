"""Vectors for the creation of range proofs (cg_range_*): a synthetic KZG key with a known trapdoor, a restatement of
`RangeProof::prove_n_bits` (creds/src/rangeproof.rs:114-339) with every random value and all three challenges explicit,
and a restatement of `verify_n_bits` (:342-424) that uses the trapdoor where the reference pairs.  Built on
oracle/bn254_oracle.py only.  The expected bytes are MSMs over the key's points; the verifier works on a proof's bytes
and the trapdoor; neither uses the other's route."""
import functools
from dataclasses import dataclass, field
from typing import List

import bn254_oracle as o

R = o.R
G1 = o.G1
N_RAND, N_RESP = 18, 6
MADE, MALFORMED = 1, 2
# the rand row, in the order the reference draws it
B, F, TM, TR, TF, G, Q = slice(0, 3), slice(3, 6), 6, 7, slice(8, 11), slice(11, 15), slice(15, 18)

fe = o.fe_bytes


def fes(xs) -> bytes:
    return b"".join(fe(x) for x in xs)


def inv(x):
    return pow(x, R - 2, R)


# ---- polynomials over Fr, little-endian coefficient lists of fixed length (leading zeros are kept) -----------------------
def p_mul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % R
    return out


def p_eval(p, z):
    acc = 0
    for c in reversed(p):
        acc = (acc * z + c) % R
    return acc


def p_div_linear(p, z):
    """p / (X - z): (quotient of len(p) - 1 coefficients, remainder = p(z))"""
    q = [0] * (len(p) - 1)
    carry = 0
    for i in range(len(p) - 1, 0, -1):
        carry = (p[i] + z * carry) % R
        q[i - 1] = carry
    return q, (p[0] + z * carry) % R


def p_div_vanishing(p, n):
    """p / (X^n - 1): (quotient of len(p) - n coefficients, remainder of n)"""
    q = [0] * (len(p) - n)
    for i in range(len(q) - 1, -1, -1):
        q[i] = (p[i + n] + (q[i + n] if i + n < len(q) else 0)) % R
    return q, [(p[i] + q[i]) % R if i < len(q) else p[i] for i in range(n)]


@dataclass
class Polys:
    n: int
    g: List[int]                 # g~, n + 3 coefficients
    q1: List[int] = None
    q2: List[int] = None
    q3: List[int] = None
    rem: tuple = ()              # the three remainders: all zero iff m < 2^n
    q: List[int] = None          # 2n + 4
    w_hat: List[int] = None      # 2n + 4
    rand_w: List[int] = None     # 3
    wit: list = field(default_factory=list)       # the witness quotients of proof_g, proof_gw, proof_w_hat
    blind: list = field(default_factory=list)     # the blinded quotients
    evals: list = field(default_factory=list)     # eval_g, eval_gw, eval_w_hat
    vs: list = field(default_factory=list)        # random_v of each


def g_blinded(n, m, b):
    bits = [(m >> i) & 1 for i in range(n)]
    ev = [0] * n
    ev[n - 1] = bits[n - 1]
    for i in range(n - 2, -1, -1):
        ev[i] = (2 * ev[i + 1] + bits[i]) % R
    g = o.ifft(ev) + [0, 0, 0]
    for i in range(3):
        g[i] = (g[i] - b[i]) % R
        g[n + i] = (g[n + i] + b[i]) % R
    return g


def polys(n, m, rand, c=None, rho=None) -> Polys:
    """the polynomial stage: g~ always, q with c, the openings with rho"""
    w = o.root_of_unity(n)
    wl = pow(w, n - 1, R)
    P = Polys(n, g_blinded(n, m, rand[B]))       # from m's low n bits, as the reference takes them
    g = P.g
    if c is None:
        return P
    P.q1, r1 = p_div_linear([(g[0] - m) % R] + g[1:], 1)
    one_minus = lambda p: [(1 - p[0]) % R] + [(-x) % R for x in p[1:]]
    P.q2, r2 = p_div_linear(p_mul(g, one_minus(g)), wl)
    h = [(x - 2 * x * pow(w, i, R)) % R for i, x in enumerate(g)]
    P.q3, r3 = p_div_vanishing(p_mul(p_mul(h, one_minus(h)), [(-wl) % R, 1]), n)
    P.rem = (r1, r2, tuple(r3))
    q3 = P.q3 + [0] * (2 * n + 4 - len(P.q3))
    q1 = P.q1 + [0] * (2 * n + 4 - len(P.q1))
    P.q = [(q1[i] + c * P.q2[i] + c * c * q3[i]) % R for i in range(2 * n + 4)]
    if rho is None:
        return P
    q_coeff = (pow(rho, n, R) - 1) % R
    f_coeff = q_coeff * inv((rho - 1) % R) % R
    P.w_hat = [(q_coeff * x) % R for x in P.q]
    P.w_hat[0] = (P.w_hat[0] + f_coeff * m) % R
    P.rand_w = [(f_coeff * a + q_coeff * b) % R for a, b in zip(rand[F], rand[Q])]
    for p, z, rnd in ((g, rho, rand[G]), (g, rho * w % R, rand[G]), (P.w_hat, rho, P.rand_w)):
        wit, ev = p_div_linear(p, z)
        bl, v = p_div_linear(list(rnd), z)
        P.wit.append(wit)
        P.blind.append(bl)
        P.evals.append(ev)
        P.vs.append(v)
    return P


# ---- the key ---------------------------------------------------------------------------------------------------------------
@dataclass
class Key:
    n_bits: int
    s_g: int
    s_gamma: int
    beta: int
    pg: list                     # powers_of_g, affine
    pgam: list                   # powers_of_gamma_g
    data: bytes                  # range_pk.bin

    def table(self, P):
        return _table(P)


@functools.lru_cache(maxsize=None)
def _table(P):
    return G1.fixed_base_table(P, 4, 256)


def g1(k):
    return G1.to_affine(G1.mul_affine(o.G1_GEN, k % R))


def pk_bytes(pg, pgam) -> bytes:
    """`Powers` as write_to_file writes it: two Vec<G1Affine>, uncompressed (data_structures.rs:144-176)"""
    return b"".join(len(v).to_bytes(8, "little") + b"".join(o.g1_uncompressed(P) for P in v) for v in (pg, pgam))


@functools.lru_cache(maxsize=None)
def key(n_bits, seed=1, n_g=None, n_gamma=4) -> Key:
    import random
    rng = random.Random(1000 * seed + n_bits)
    s_g, s_gamma, beta = (rng.randrange(1, R) for _ in range(3))
    n_g = 2 * n_bits + 4 if n_g is None else n_g
    pg = [g1(s_g * pow(beta, i, R)) for i in range(n_g)]
    pgam = [g1(s_gamma * pow(beta, i, R)) for i in range(n_gamma)]
    return Key(n_bits, s_g, s_gamma, beta, pg, pgam, pk_bytes(pg, pgam))


def msm(points, scalars):
    """sum s_i P_i over actual points (a 4-bit table per point, cached), affine or None"""
    acc = G1.jac_infinity()
    for P, s in zip(points, scalars):
        if P is not None and s % R:
            acc = G1.add(acc, G1.fixed_base_mul(_table(P), s % R))
    return G1.to_affine(acc)


# ---- prove_n_bits ----------------------------------------------------------------------------------------------------------
@dataclass
class Made:
    m: int
    r: int
    rand: List[int]
    ok: tuple = (True, True, True)     # per call: made or malformed
    com_f: tuple = None
    com_g: tuple = None
    k: list = None
    com_q: tuple = None
    evals: list = None
    W: list = None
    vs: list = None
    s: list = None
    c_dleq: int = 0
    c: int = 0
    rho: int = 0


def is_malformed(n, m, r, rand, c=None, rho=None) -> bool:
    vals = [m, r] + list(rand) + [x for x in (c, rho) if x is not None]
    if any(v >= R for v in vals) or m >= (1 << n):
        return True
    if not any(rand[F]) or not any(rand[G]) or not any(rand[Q]):
        return True
    return rho is not None and pow(rho, n, R) == 1


def prove(K: Key, bases, m, r, rand, c_dleq, c, rho) -> Made:
    """every output of the three calls and the responses; a call whose inputs are malformed leaves its fields None"""
    n = K.n_bits
    out = Made(m, r, list(rand), c_dleq=c_dleq, c=c, rho=rho)
    out.ok = (not is_malformed(n, m, r, rand), not is_malformed(n, m, r, rand, c), not is_malformed(n, m, r, rand, c, rho))
    if out.ok[0]:
        P = polys(n, m, rand)
        out.com_f = msm([K.pg[0]] + K.pgam[:3], [m] + rand[F])
        out.com_g = msm(K.pg[:n + 3] + K.pgam[:4], P.g + rand[G])
        out.k = [msm(bases, [rand[TM], rand[TR]]), msm(K.pgam[:3] + [K.pg[0]], rand[TF] + [rand[TM]])]
        if c_dleq < R:
            nonces = [rand[TM], rand[TR]] + rand[TF] + [rand[TM]]
            secrets = [m, r] + rand[F] + [m]
            out.s = [(t - c_dleq * x) % R for t, x in zip(nonces, secrets)]
    if out.ok[1]:
        P = polys(n, m, rand, c)
        out.com_q = msm(K.pg[:2 * n + 4] + K.pgam[:3], P.q + rand[Q])
    if out.ok[2]:
        P = polys(n, m, rand, c, rho)
        out.evals, out.vs = P.evals, P.vs
        out.W = [msm(K.pg[:len(wit)] + K.pgam[:len(bl)], wit + bl) for wit, bl in zip(P.wit, P.blind)]
    return out


def pack(made):
    """(openings, rand, c, rho, c_dleq) of a batch as the header lays them out"""
    return (b"".join(fe(x.m) + fe(x.r) for x in made), b"".join(fes(x.rand) for x in made),
            fes(x.c for x in made), fes(x.rho for x in made), fes(x.c_dleq for x in made))


def expected_commit(x: Made):
    if not x.ok[0]:
        return bytes(64), bytes(64), bytes(128)
    return (o.g1_uncompressed(x.com_f), o.g1_uncompressed(x.com_g),
            b"".join(o.g1_compressed(P) for P in (x.com_f, x.com_g, x.k[0], x.k[1])))


def expected_quotient(x: Made):
    if not x.ok[1]:
        return bytes(64), bytes(32)
    return o.g1_uncompressed(x.com_q), o.g1_compressed(x.com_q)


def expected_open(x: Made):
    if not x.ok[2]:
        return bytes(96), bytes(288)
    return fes(x.evals), b"".join(o.g1_uncompressed(W) + fe(v) for W, v in zip(x.W, x.vs))


def ark_bytes(com_f, com_g, evals, proofs, com_q, c_dleq, s) -> bytes:
    """`RangeProof` serialize_uncompressed (rangeproof.rs:82-93) from the calls' bytes: written independently of api.py.
    kzg10::Proof is w ‖ Option<Fr> (a tag byte, then the value); DLogPoK is c ‖ Vec<Vec<Fr>>"""
    u64 = lambda v: int(v).to_bytes(8, "little")
    pr = lambda j: proofs[96 * j:96 * j + 64] + b"\x01" + proofs[96 * j + 64:96 * j + 96]
    ev = lambda j: evals[32 * j:32 * j + 32]
    dleq = fe(c_dleq) + u64(2) + u64(2) + fes(s[:2]) + u64(4) + fes(s[2:])
    return com_f + com_g + ev(0) + pr(0) + ev(1) + pr(1) + com_q + ev(2) + pr(2) + dleq


# ---- verify_n_bits with the trapdoor in place of the pairings ---------------------------------------------------------------
def _rd_g1(b):
    """ark-serialize uncompressed, unchecked"""
    if b[63] & 0x40:
        return None
    y = bytearray(b[32:64])
    y[31] &= 0x3F
    return int.from_bytes(b[:32], "little"), int.from_bytes(bytes(y), "little")


def _eq(J1, J2):
    return G1.to_affine(J1) == G1.to_affine(J2)


def verify(K: Key, bases, ped_com, proof: bytes, c, rho, k_bytes=None) -> bool:
    """`verify_n_bits` on a serialized RangeProof, given the two challenges the host's transcript produced (this package
    ships no Merlin): the three openings as (beta - z) W == com - eval g - v gamma_g, the eval_w identity, and the DLEQ:
    s_13 == s_00 and, when k_bytes is given, its recomputed k_i equal to the ones that were absorbed"""
    n = K.n_bits
    w = o.root_of_unity(n)
    at = 0

    def take(k):
        nonlocal at
        at += k
        return proof[at - k:at]

    def take_proof():
        W = _rd_g1(take(64))
        assert take(1) == b"\x01"
        return W, int.from_bytes(take(32), "little")

    fr = lambda: int.from_bytes(take(32), "little")
    com_f, com_g = _rd_g1(take(64)), _rd_g1(take(64))
    eval_g, proof_g, eval_gw, proof_gw = fr(), take_proof(), fr(), take_proof()
    com_q = _rd_g1(take(64))
    eval_w, proof_w = fr(), take_proof()
    c_dleq = fr()
    assert int.from_bytes(take(8), "little") == 2
    s = [[fr() for _ in range(int.from_bytes(take(8), "little"))] for _ in range(2)]
    assert at == len(proof) and [len(x) for x in s] == [2, 4]

    q_coeff = (pow(rho, n, R) - 1) % R
    f_coeff = q_coeff * inv((rho - 1) % R) % R
    com_w = G1.to_affine(G1.add(G1.mul_affine(com_f, f_coeff), G1.mul_affine(com_q, q_coeff)))
    g0, gam0 = K.pg[0], K.pgam[0]
    for com, z, ev, (W, v) in ((com_g, rho, eval_g, proof_g), (com_g, rho * w % R, eval_gw, proof_gw), (com_w, rho, eval_w, proof_w)):
        lhs = G1.mul_affine(W, (K.beta - z) % R)
        rhs = G1.add(G1.to_jac(com), G1.add(G1.mul_affine(g0, (-ev) % R), G1.mul_affine(gam0, (-v) % R)))
        if not _eq(lhs, rhs):
            return False
    wl = pow(w, n - 1, R)
    w1 = eval_g * q_coeff % R * inv((rho - 1) % R) % R
    w2 = eval_g * (1 - eval_g) % R * q_coeff % R * inv((rho - wl) % R) % R
    d = (eval_g - 2 * eval_gw) % R
    w3 = d * (1 - d) % R * (rho - wl) % R
    if (w1 + c * w2 + c * c * w3 - eval_w) % R:
        return False
    if s[0][0] != s[1][3]:
        return False
    if k_bytes is not None:
        ks = [G1.add(G1.add(G1.mul_affine(bases[0], s[0][0]), G1.mul_affine(bases[1], s[0][1])), G1.mul_affine(ped_com, c_dleq)),
              G1.mul_affine(com_f, c_dleq)]
        for P, x in zip(K.pgam[:3] + [K.pg[0]], s[1]):
            ks[1] = G1.add(ks[1], G1.mul_affine(P, x))
        if b"".join(o.g1_compressed(G1.to_affine(J)) for J in ks) != bytes(k_bytes):
            return False
    return True
