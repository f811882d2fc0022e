"""The BN254 half of a device proof in pure Python, sharing no code with the library: `DeviceProof::prove`
(creds/src/device.rs:98-165) with every random scalar and h_Q given, and `DeviceProof::verify` (:168-213) short of pi2, read
from the BYTES a verifier receives.  Over oracle/bn254_oracle.py, tests/merlin_vectors.py and hashlib.  Keys come from
tests/verify_vectors.py's synthetic scalars, so every discrete logarithm is known and points can be steered.

The text forms SHA-256 is fed (`to_string()` of arkworks 0.4 values) are restated from the 0.4 sources and UNVERIFIED until an
arkworks-made DeviceProof meets this code; each rule is one function here (dec, point_text) and one in
csrc/device_link.hpp."""
import hashlib
from types import SimpleNamespace

import bn254_oracle as o
import merlin_vectors as MV
import verify_vectors as V

Q, R = o.Q, o.R
CONTEXT_E = b"computing challenge for linking proof"
CONTEXT_PI0 = b"creating sigma proof pi0 for linking proof"
CONTEXT_PI1 = b"creating sigma proof pi1 for linking proof"
REJECT, ACCEPT, MALFORMED = 0, 1, 2
REVEALED, HIDDEN, COMMITTED = 0, 1, 2


# ---- the text forms ----------------------------------------------------------------------------------------------------------
def dec(v: int) -> str:
    """ark-ff 0.4 `Display for Fp`: into_bigint().to_string().trim_start_matches('0') - zero is the empty string"""
    return str(int(v)).lstrip("0")


def point_text(P) -> str:
    """ark-ec 0.4 `Display for Affine`; `Projective` prints its affine form"""
    return "infinity" if P is None else "(%s, %s)" % (dec(P[0]), dec(P[1]))


def message(c0: int, com0, com1, comz, h_q: bytes) -> bytes:
    return CONTEXT_E + (dec(c0) + point_text(com0) + point_text(com1) + point_text(comz)).encode() + bytes(h_q)


def challenge_digest(c0, com0, com1, comz, h_q) -> bytes:
    return hashlib.sha256(message(c0, com0, com1, comz, h_q)).digest()


def e_of(digest: bytes):
    return int.from_bytes(digest[:16], "little"), int.from_bytes(digest[16:], "little")


# ---- the group -----------------------------------------------------------------------------------------------------------------
def mul(P, k):
    return None if P is None else o.G1.to_affine(o.G1.mul_affine(P, k % R))


def add(P, S):
    if P is None:
        return S
    if S is None:
        return P
    return o.G1.to_affine(o.G1.add_affine(o.G1.to_jac(P), S))


def neg(P):
    return None if P is None else o.G1.neg_affine(P)


def msm(points, scalars):
    acc = None
    for P, k in zip(points, scalars):
        acc = add(acc, mul(P, k))
    return acc


def dlog_challenge(context, bases, ks, ys) -> int:
    st = [([o.g1_compressed(b) for b in bs], o.g1_compressed(k), o.g1_compressed(y)) for bs, k, y in zip(bases, ks, ys)]
    return MV.to_int(MV.dlog_challenge(context, st))


def dlog_prove(context, ys, bases, scalars, nonces):
    """DLogPoK::prove (dlog.rs:39-115) with the nonces given, equal positions included -> (c, s)"""
    ks = [msm(bs, ns) for bs, ns in zip(bases, nonces)]
    c = dlog_challenge(context, bases, ks, ys)
    return c, [[(n - c * x) % R for n, x in zip(ns, xs)] for ns, xs in zip(nonces, scalars)]


def dlog_verify(context, c, s, bases, ys, eq_pos=None) -> bool:
    """DLogPoK::verify (dlog.rs:117-175)"""
    ks = [msm(list(bs) + [y], list(si) + [c]) for bs, si, y in zip(bases, s, ys)]
    if eq_pos is not None and any(s[0][i] != s[1][j] for i, j in eq_pos):
        return False
    return dlog_challenge(context, bases, ks, ys) == c


# ---- keys ------------------------------------------------------------------------------------------------------------------------
def make_key(io_types, pos0, pos1, seed):
    """a synthetic verifying key of len(io_types) inputs with known scalars: g = gamma_abc_g1[pos0 + 1], g' =
    gamma_abc_g1[pos1 + 1], h = delta_g1"""
    ell = len(io_types)
    rng, sc = V.synthetic_scalars(ell, seed)
    vk = V.synthetic_vk(*sc[:4], sc[4])
    com = [i for i, t in enumerate(io_types) if t == COMMITTED]
    return SimpleNamespace(io=list(io_types), pos0=pos0, pos1=pos1, sc=sc, vk=vk, rng=rng, com=com, ci0=com.index(pos0), ci1=com.index(pos1),
                           kg=sc[4][pos0 + 1], kgp=sc[4][pos1 + 1], kh=sc[3], g=vk["gamma_abc_g1"][pos0 + 1], gp=vk["gamma_abc_g1"][pos1 + 1],
                           h=vk["delta_g1"])


# ---- prove -----------------------------------------------------------------------------------------------------------------------
def prove(key, q0, r0, q1, r1_orig, r1, z, tz, nonces0, nonces1, h_q, eq_nonce=None):
    """The BN254 half of DeviceProof::prove.  com0 = q0 g + r0 h and com1_orig = q1 g' + r1_orig h are the showing's committed
    points; r1 blinds the re-committed com1, (z, tz) open comz.  nonces0 = (a, b, d): pi0's r[0] = [a, b], r[1] = [a, d]
    (eq_pos (0, 0); eq_nonce replaces r[1][0], which an honest prover never does); nonces1 = (n0, n1, n2): pi1's r[0] = [n0],
    r[1] = [n1, n2].  Returns a record of ints and affine points."""
    g, gp, h = key.g, key.gp, key.h
    com0, com1_orig = msm([g, h], [q0, r0]), msm([gp, h], [q1, r1_orig])
    com1, comz = msm([g, h], [q1, r1]), msm([g, h], [z, tz])
    a, b, d = nonces0
    pi0_c, s0 = dlog_prove(CONTEXT_PI0, [com1_orig, com1], [[gp, h], [g, h]], [[q1, r1_orig], [q1, r1]],
                           [[a, b], [a if eq_nonce is None else eq_nonce, d]])
    digest = challenge_digest(pi0_c, com0, com1, comz, h_q)
    e1, e2 = e_of(digest)
    m = (q0 + q1 * e1 + z * e2) % R
    r = (r0 + r1 * e1 + tz * e2) % R
    lhs1 = add(add(add(com0, mul(com1, e1)), mul(comz, e2)), neg(mul(g, m)))
    assert lhs1 == mul(h, r)
    n0, n1, n2 = nonces1
    pi1_c, s1 = dlog_prove(CONTEXT_PI1, [lhs1, comz], [[h], [g, h]], [[r], [z, tz]], [[n0], [n1, n2]])
    return SimpleNamespace(com0=com0, com1_orig=com1_orig, com1=com1, comz=comz, h_q=bytes(h_q), m=m, pi0_c=pi0_c, pi0_s=s0[0] + s0[1], pi1_c=pi1_c,
                           pi1_s=s1[0] + s1[1], digest=digest)


def random_record(key, rng, h_len=32, **kw):
    s = lambda: rng.randrange(1, R)
    args = dict(q0=s(), r0=s(), q1=s(), r1_orig=s(), r1=s(), z=s(), tz=s(), nonces0=(s(), s(), s()), nonces1=(s(), s(), s()),
                h_q=bytes(rng.randrange(256) for _ in range(h_len)))
    args.update(kw)
    return prove(key, **args)


# ---- the bytes -------------------------------------------------------------------------------------------------------------------
def fe(v) -> bytes:
    return int(v).to_bytes(32, "little")


def record_bytes(key, rec, others=None):
    """one row of every array as the entry takes it: (committed, com1, comz, h_q, m, pi0_c, pi0_s, pi1_c, pi1_s).  committed
    holds com0 and com1_orig at the committed indices of pos0 and pos1; `others` fills the remaining committed points.
    A field of rec that already is bytes goes in as it stands (malformed rows)."""
    pt = lambda P: P if isinstance(P, (bytes, bytearray)) else o.g1_uncompressed(P)
    sc = lambda v: v if isinstance(v, (bytes, bytearray)) else fe(v)
    committed = [pt(P) for P in (others or [o.G1_GEN] * len(key.com))]
    committed[key.ci0], committed[key.ci1] = pt(rec.com0), pt(rec.com1_orig)
    return (b"".join(committed), pt(rec.com1), pt(rec.comz), bytes(rec.h_q), sc(rec.m), sc(rec.pi0_c), b"".join(sc(x) for x in rec.pi0_s),
            sc(rec.pi1_c), b"".join(sc(x) for x in rec.pi1_s))


def checked_g1(b: bytes):
    """ark's checked deserialisation of an uncompressed G1 point -> (ok, point)"""
    flags = b[63] >> 6
    x, y = int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little") & ((1 << 254) - 1)
    if flags == 3 or x >= Q or y >= Q:
        return False, None
    if flags == 1:
        return True, None
    return (y * y - x * x * x - 3) % Q == 0, (x, y)


def verify(key, row):
    """DeviceProof::verify short of pi2 on one row of record_bytes -> (verdict, (pi0 part, pi1 part), digest bytes).  A
    malformed row has parts (MALFORMED, MALFORMED) and a digest of zero bytes."""
    committed, com1_b, comz_b, h_q, m_b, c0_b, s0_b, c1_b, s1_b = row
    pts = [checked_g1(committed[64 * i:64 * i + 64]) for i in (key.ci0, key.ci1)] + [checked_g1(com1_b), checked_g1(comz_b)]
    ints = lambda b: [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]
    m, c0, c1, s0, s1 = ints(m_b)[0], ints(c0_b)[0], ints(c1_b)[0], ints(s0_b), ints(s1_b)
    if not all(ok for ok, _ in pts) or any(v >= R for v in [m, c0, c1] + s0 + s1):
        return MALFORMED, (MALFORMED, MALFORMED), bytes(32)
    com0, com1_orig, com1, comz = (P for _, P in pts)
    g, gp, h = key.g, key.gp, key.h
    ok0 = dlog_verify(CONTEXT_PI0, c0, [s0[:2], s0[2:]], [[gp, h], [g, h]], [com1_orig, com1], eq_pos=[(0, 0)])
    digest = challenge_digest(c0, com0, com1, comz, h_q)
    e1, e2 = e_of(digest)
    lhs1 = add(add(add(com0, mul(com1, e1)), mul(comz, e2)), neg(mul(g, m)))
    ok1 = dlog_verify(CONTEXT_PI1, c1, [s1[:1], s1[1:]], [[h], [g, h]], [lhs1, comz])
    return (ACCEPT if ok0 and ok1 else REJECT), (ACCEPT if ok0 else REJECT, ACCEPT if ok1 else REJECT), digest


def pack(rows):
    """rows of record_bytes -> the nine flat byte strings"""
    return tuple(b"".join(r[i] for r in rows) for i in range(9))
