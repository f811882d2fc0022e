"""Vectors for the verification of range proofs (cg_range_verify_batch): the 640-byte `RangeProofVK` of
tests/range_vectors.py's synthetic key, a restatement of `RangeProof::verify_n_bits` (creds/src/rangeproof.rs:342-424) with
the two randomizers of `KZG10::batch_check` (forks/ark-poly-commit/src/kzg10/mod.rs:357-411) explicit, and a forger that
uses the key's trapdoor to make proofs the reference accepts around any chosen commitments, challenges and evaluations.

The pairing check is restated by two routes that share no code with each other or with the library:
  (a) the trapdoor:  total_c == beta total_w in G1 (beta_h = O: total_c == O)
  (b) the pairing:   oracle/ark_files.py's g2_prepare, multi_miller_loop and final_exponentiation over
                     (-total_w, beta_h), (total_c, h), a pair with an O point dropped
Route (a) gives the expected verdict of every row; route (b) is slow and pins, on a handful of rows, which side of the
equation and which sign the reference uses.  total_c and total_w are formed as batch_check forms them, term by term per
opening; the library merges scalars instead, and `merged_scalars` restates that merging for the scalar stage's test.
Built on range_vectors.py and oracle/ only."""
from dataclasses import dataclass, replace
from typing import List

import ark_files as AF
import bn254_oracle as o
import range_vectors as RV

R, Q = o.R, o.Q
G1, G2 = o.G1, o.G2
REJECT, ACCEPT, MALFORMED = 0, 1, 2
inv = RV.inv
fe, fes = RV.fe, RV.fes
unc = o.g1_uncompressed


def vk_bytes(K: RV.Key, h_scalar=1, beta_h_inf=False) -> bytes:
    """range_vk.bin: g | gamma_g | h | beta_h (kzg10/data_structures.rs:217-264), then com_f_basis = gamma_g[0..2], g[0]
    (rangeproof.rs:42-47) as four points without a length"""
    h, beta_h = key_g2(K, h_scalar, beta_h_inf)
    return (unc(K.pg[0]) + unc(K.pgam[0]) + o.g2_uncompressed(h) + o.g2_uncompressed(beta_h)
            + b"".join(unc(P) for P in K.pgam[:3] + [K.pg[0]]))


def key_g2(K, h_scalar=1, beta_h_inf=False):
    h = G2.to_affine(G2.mul_affine(o.G2_GEN, h_scalar % R))
    return h, None if beta_h_inf else G2.to_affine(G2.mul_affine(h, K.beta))


@dataclass
class Row:
    """one showing as the call takes it: points as their 64 bytes, scalars as ints (any value: >= r reaches the check)"""
    ped_com: bytes
    com_f: bytes
    com_g: bytes
    com_q: bytes
    evals: List[int]
    W: List[bytes]
    vs: List[int]
    c: int
    rho: int
    r1: int
    r2: int
    pok_c: int
    s: List[int]

    def but(self, **kw):
        return replace(self, **kw)

    def with_item(self, name, i, v):
        x = list(getattr(self, name))
        x[i] = v
        return replace(self, **{name: x})


def pack(rows):
    """the call's arrays in the header's order after `slot`: ped_com .. pok_s"""
    j = lambda f: b"".join(f(x) for x in rows)
    return (j(lambda x: x.ped_com), j(lambda x: x.com_f), j(lambda x: x.com_g), j(lambda x: x.com_q), j(lambda x: fes(x.evals)),
            j(lambda x: b"".join(W + fe(v) for W, v in zip(x.W, x.vs))), j(lambda x: fe(x.c)), j(lambda x: fe(x.rho)),
            j(lambda x: x.r1.to_bytes(16, "little") + x.r2.to_bytes(16, "little")), j(lambda x: fe(x.pok_c)), j(lambda x: fes(x.s)))


def from_made(x: RV.Made, ped_com, r1, r2) -> Row:
    """a proof of range_vectors.prove as a row"""
    return Row(unc(ped_com), unc(x.com_f), unc(x.com_g), unc(x.com_q), list(x.evals), [unc(W) for W in x.W], list(x.vs), x.c, x.rho,
               r1, r2, x.c_dleq, list(x.s))


# ---- ark's checked deserialisation of an uncompressed G1 point ---------------------------------------------------------------
def rd_g1_checked(b):
    """(ok, point or None)"""
    flags = b[63] & 0xC0
    x = int.from_bytes(b[:32], "little")
    y = int.from_bytes(b[32:63] + bytes([b[63] & 0x3F]), "little")
    if flags == 0xC0 or x >= Q or y >= Q:
        return False, None
    if flags == 0x40:
        return True, None
    return (y * y - x * x * x - 3) % Q == 0, (x, y)


# ---- steps 2-5 ----------------------------------------------------------------------------------------------------------------
def coeffs(n, rho):
    q_coeff = (pow(rho, n, R) - 1) % R
    return q_coeff, q_coeff * inv((rho - 1) % R) % R


def identity_holds(n, x: Row) -> bool:
    wl = pow(o.root_of_unity(n), n - 1, R)
    q_coeff, _ = coeffs(n, x.rho)
    eg, egw, ew = x.evals
    w1 = eg * q_coeff % R * inv((x.rho - 1) % R) % R
    w2 = eg * (1 - eg) % R * q_coeff % R * inv((x.rho - wl) % R) % R
    d = (eg - 2 * egw) % R
    w3 = d * (1 - d) % R * (x.rho - wl) % R
    return (w1 + x.c * w2 + x.c * x.c * w3 - ew) % R == 0


def totals(K, n, x: Row, pts):
    """(total_c, total_w), affine, formed as batch_check forms them"""
    com_f, com_g, com_q, W = pts["com_f"], pts["com_g"], pts["com_q"], pts["W"]
    w = o.root_of_unity(n)
    q_coeff, f_coeff = coeffs(n, x.rho)
    com_w = G1.to_affine(G1.add(G1.mul_affine(com_f, f_coeff), G1.mul_affine(com_q, q_coeff)))
    total_c, total_w = G1.jac_infinity(), G1.jac_infinity()
    g_mult = gamma_mult = 0
    for C, z, v, Wi, rv, rz in zip((com_g, com_g, com_w), (x.rho, x.rho * w % R, x.rho), x.evals, W, x.vs, (1, x.r1, x.r2)):
        temp = G1.add_affine(G1.mul_affine(Wi, z), C)
        g_mult = (g_mult + rz * v) % R
        gamma_mult = (gamma_mult + rz * rv) % R
        total_c = G1.add(total_c, G1.mul(temp, rz))
        total_w = G1.add(total_w, G1.mul_affine(Wi, rz))
    total_c = G1.add(total_c, G1.neg(G1.mul_affine(K.pg[0], g_mult)))
    total_c = G1.add(total_c, G1.neg(G1.mul_affine(K.pgam[0], gamma_mult)))
    return G1.to_affine(total_c), G1.to_affine(total_w)


def pairing_by_trapdoor(K, total_c, total_w, beta_h_inf=False) -> bool:
    """route (a): e(-total_w, beta h) e(total_c, h) = e(total_c - beta total_w, h), h != O"""
    if beta_h_inf:
        return total_c is None
    return G1.to_affine(G1.mul_affine(total_w, K.beta)) == total_c


def pairing_by_ark(K, total_c, total_w, h_scalar=1, beta_h_inf=False) -> bool:
    """route (b): E::multi_pairing([-total_w, total_c], [prepared_beta_h, prepared_h]).is_one() (kzg10/mod.rs:397-407)"""
    h, beta_h = key_g2(K, h_scalar, beta_h_inf)
    f = AF.multi_miller_loop([(G1.neg_affine(total_w), AF.g2_prepare(beta_h)), (total_c, AF.g2_prepare(h))])
    return AF.final_exponentiation(f) == o._f12_one()


def parse(x: Row, pok=True):
    """None for a malformed showing, else its points"""
    names = ["com_f", "com_g", "com_q"] + (["ped_com"] if pok else [])
    pts, ok = {}, True
    for name in names:
        good, pts[name] = rd_g1_checked(getattr(x, name))
        ok = ok and good
    pts["W"] = []
    for b in x.W:
        good, P = rd_g1_checked(b)
        ok = ok and good
        pts["W"].append(P)
    scalars = list(x.evals) + list(x.vs) + [x.c, x.rho] + ([x.pok_c] + list(x.s) if pok else [])
    return pts if ok and all(0 <= v < R for v in scalars) else None


def dleq_k(K, bases, x: Row, pts):
    """k_0, k_1 of DLogPoK::verify (creds/src/dlog.rs:135-145), affine"""
    k0 = G1.add(G1.to_jac(RV.msm(bases, x.s[:2])), G1.mul_affine(pts["ped_com"], x.pok_c))
    k1 = G1.add(G1.to_jac(RV.msm(K.pgam[:3] + [K.pg[0]], x.s[2:])), G1.mul_affine(pts["com_f"], x.pok_c))
    return G1.to_affine(k0), G1.to_affine(k1)


def expected(K, bases, x: Row, pok=True, beta_h_inf=False, pairing=pairing_by_trapdoor):
    """(verdict, k_out bytes or None) of one showing"""
    n = K.n_bits
    pts = parse(x, pok)
    wl = pow(o.root_of_unity(n), n - 1, R)
    if pts is None or x.rho in (1, wl):
        return MALFORMED, bytes(64) if pok else None
    ok = pairing(K, *totals(K, n, x, pts), beta_h_inf=beta_h_inf) and identity_holds(n, x)
    if not pok:
        return (ACCEPT if ok else REJECT), None
    ok = ok and x.s[0] == x.s[5]
    return (ACCEPT if ok else REJECT), b"".join(o.g1_compressed(P) for P in dleq_k(K, bases, x, pts))


# ---- the scalar stage's merged scalars (csrc/rangeverify.hpp), restated ------------------------------------------------------
def merged_scalars(n, x: Row):
    """the ten scalars in the header's order: (1 + r_1), r_2 f, r_2 q, rho, r_1 rho w, r_2 rho | r_1, r_2 | Σ r_i v_i, Σ r_i rv_i"""
    w = o.root_of_unity(n)
    q_coeff, f_coeff = coeffs(n, x.rho)
    rz = (1, x.r1, x.r2)
    return [1 + x.r1, x.r2 * f_coeff % R, x.r2 * q_coeff % R, x.rho, x.r1 * x.rho * w % R, x.r2 * x.rho % R, x.r1, x.r2,
            sum(a * b for a, b in zip(rz, x.evals)) % R, sum(a * b for a, b in zip(rz, x.vs)) % R]


# ---- the forger -----------------------------------------------------------------------------------------------------------------
def forge(K, a_f, a_g, a_q, c, rho, eval_g, eval_gw, vs, r1, r2, ped_com=None, pok_c=0, s=(0,) * 6) -> Row:
    """a proof around com_f = a_f G, com_g = a_g G, com_q = a_q G that the reference accepts for ANY randomizers: eval_w^ from
    the identity, W_i = (C_i - v_i g - random_v_i gamma_g)/(beta - z_i) by the trapdoor.  A wrong sum in the verifier flips
    the verdict, where garbage would be rejected either way."""
    n = K.n_bits
    w = o.root_of_unity(n)
    wl = pow(w, n - 1, R)
    q_coeff, f_coeff = coeffs(n, rho)
    d = (eval_g - 2 * eval_gw) % R
    eval_w = (eval_g * f_coeff + c * eval_g * (1 - eval_g) % R * q_coeff % R * inv((rho - wl) % R) + c * c * d % R * (1 - d) % R * (rho - wl)) % R
    evals = [eval_g % R, eval_gw % R, eval_w]
    logs = [w_log(K, a_C, z, v, rv) for a_C, z, v, rv in zip((a_g, a_g, (f_coeff * a_f + q_coeff * a_q) % R), (rho, rho * w % R, rho), evals, vs)]
    return Row(unc(ped_com), unc(RV.g1(a_f)), unc(RV.g1(a_g)), unc(RV.g1(a_q)), evals, [unc(RV.g1(l)) for l in logs], list(vs), c, rho,
               r1, r2, pok_c, list(s))


def w_log(K, a_C, z, v, rv):
    """the discrete log of the W that opens a_C G at z to v with random_v rv"""
    return (a_C - v * K.s_g - rv * K.s_gamma) * inv((K.beta - z) % R) % R


def rv_for_w_log(K, a_C, z, v, log_w):
    """the random_v that makes that W equal log_w G"""
    return (a_C - v * K.s_g - log_w * (K.beta - z)) * inv(K.s_gamma) % R


# ---- rows both test files use ---------------------------------------------------------------------------------------------------
B0, B1 = 0x1234567, 0x89ABCDEF123        # the Pedersen bases' scalars: B_i = b_i G


def bases_of(b0=B0, b1=B1):
    return [RV.g1(b0), RV.g1(b1)]


def valid_row(K, bases, rng, m=None, rand=None, **kw):
    """a proof range_vectors.prove makes, with random challenges and randomizers; kw overrides c, rho or c_dleq"""
    d = dict(c=rng.randrange(R), rho=rng.randrange(R), c_dleq=rng.randrange(R))
    d.update(kw)
    m = rng.randrange(1 << K.n_bits) if m is None else m
    r = rng.randrange(R)
    rand = [rng.randrange(R) for _ in range(RV.N_RAND)] if rand is None else rand
    x = RV.prove(K, bases, m, r, rand, d["c_dleq"], d["c"], d["rho"])
    assert x.ok == (True, True, True)
    return from_made(x, RV.msm(bases, [m, r]), rng.getrandbits(128), rng.getrandbits(128)), x


def forged_row(K, rng, **kw):
    """forge() with everything the caller leaves out drawn at random; the DLEQ part is any responses with s_13 = s_00"""
    s = [rng.randrange(R) for _ in range(5)]
    d = dict(a_f=rng.randrange(R), a_g=rng.randrange(R), a_q=rng.randrange(R), c=rng.randrange(R), rho=rng.randrange(R),
             eval_g=rng.randrange(R), eval_gw=rng.randrange(R), vs=[rng.randrange(R) for _ in range(3)], r1=rng.getrandbits(128),
             r2=rng.getrandbits(128), ped_com=RV.g1(rng.randrange(R)), pok_c=rng.randrange(R), s=s + [s[0]])
    d.update(kw)
    return forge(K, **d)


def all_infinity_row(r1=5, r2=7) -> Row:
    """every point O, every scalar 0: m = 0 with no blinding.  total_c = total_w = O: both pairs are dropped"""
    O = unc(None)
    return Row(O, O, O, O, [0, 0, 0], [O, O, O], [0, 0, 0], 0, 0, r1, r2, 0, [0] * 6)


def cancelling_rows(x: Row, delta):
    """proof_g's random_v shifted by -r_1 delta and proof_gw's by delta: Σ r_i random_v_i is unchanged under x's r_1
    (accepted, as the reference accepts it with that randomizer) and changes under r_1 + 1 (rejected)"""
    a = x.with_item("vs", 0, (x.vs[0] - x.r1 * delta) % R).with_item("vs", 1, (x.vs[1] + delta) % R)
    return a, a.but(r1=a.r1 + 1)


def total_w_zero_rows(K, rng):
    """forged openings with W_g = -(r_1 W_gw + r_2 W_w^): total_w = O and total_c = O (accepted, both pairs dropped); the
    same points with proof_gw's random_v off by one: total_w = O, total_c != O (rejected)"""
    n = K.n_bits
    a_f, a_g, a_q = (rng.randrange(R) for _ in range(3))
    x = forged_row(K, rng, a_f=a_f, a_g=a_g, a_q=a_q)
    w = o.root_of_unity(n)
    q_coeff, f_coeff = coeffs(n, x.rho)
    l1 = w_log(K, a_g, x.rho * w % R, x.evals[1], x.vs[1])
    l2 = w_log(K, (f_coeff * a_f + q_coeff * a_q) % R, x.rho, x.evals[2], x.vs[2])
    l0 = -(x.r1 * l1 + x.r2 * l2) % R
    good = x.with_item("vs", 0, rv_for_w_log(K, a_g, x.rho, x.evals[0], l0)).with_item("W", 0, unc(RV.g1(l0)))
    return good, good.with_item("vs", 1, (good.vs[1] + 1) % R)


def identity_breaker(K, rng) -> Row:
    """three valid openings whose evaluations miss the identity by one: the pairing check passes, the identity fails"""
    n = K.n_bits
    a_f, a_q = rng.randrange(R), rng.randrange(R)
    x = forged_row(K, rng, a_f=a_f, a_q=a_q)
    q_coeff, f_coeff = coeffs(n, x.rho)
    ew = (x.evals[2] + 1) % R
    return x.with_item("evals", 2, ew).with_item("W", 2, unc(RV.g1(w_log(K, (f_coeff * a_f + q_coeff * a_q) % R, x.rho, ew, x.vs[2]))))
