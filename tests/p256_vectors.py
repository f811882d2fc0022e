"""A pure-Python P-256 over integers, the oracle of the P-256 tests: affine formulas and pow(x, -1, p), nothing shared with
csrc/fp256.hpp, csrc/fq256.hpp or csrc/p256.hpp.

`compute_TU` and `compute_RTU` (ecdsa-pop/src/lib.rs:217-240 and :180-215) are restated with the statuses of
cg_p256_tu_batch and cg_p256_rtu_batch: where the reference panics or asserts, a row is MALFORMED or BAD_SIGNATURE and every
output of it is zero.  A point is None (the identity) or (x, y); on the wire the identity is 64 zero bytes, which is what
halo2curves' `to_affine` makes of it.  `sign` is a deterministic ECDSA signer whose nonce the caller chooses, so that a test
can place u G and v Q where it wants them."""
import random

P = 0xffffffff00000001000000000000000000000000ffffffffffffffffffffffff
N = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551
A = P - 3
B = 0x5ac635d8aa3a93e7b3ebbd55769886bc651d06b0cc53b0f63bce3c3e27d2604b
G = (0x6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296,
     0x4fe342e2fe1a7f9b8ee7eb4a7c0f9e162bce33576b315ececbb6406837bf51f5)

MADE, MALFORMED, BAD_SIGNATURE = 1, 2, 3
ZERO_POINT = bytes(64)


def on_curve(pt):
    if pt is None:
        return True
    x, y = pt
    return 0 <= x < P and 0 <= y < P and (y * y - (x * x * x + A * x + B)) % P == 0


def neg(pt):
    return None if pt is None else (pt[0], (P - pt[1]) % P)


def add(p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = (3 * x1 * x1 + A) * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def mul(k, pt):
    k %= N
    acc = None
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt = add(pt, pt)
        k >>= 1
    return acc


def be(v):
    return int(v).to_bytes(32, "big")


def point_bytes(pt):
    return ZERO_POINT if pt is None else be(pt[0]) + be(pt[1])


def _checked_point(xy):
    """x ‖ y, 64 bytes big-endian -> the point, or None if a coordinate is >= p or the point is off the curve"""
    x, y = int.from_bytes(xy[:32], "big"), int.from_bytes(xy[32:64], "big")
    if x >= P or y >= P or not on_curve((x, y)):
        return None
    return x, y


def compute_tu(r_xy, digest):
    """-> (status, t_xy, u_xy)"""
    bad = (MALFORMED, ZERO_POINT, ZERO_POINT)
    R = _checked_point(r_xy)
    if R is None:
        return bad
    r, d = R[0] % N, int.from_bytes(digest, "big") % N
    if r == 0:
        return bad
    r_inv = pow(r, -1, N)
    return MADE, point_bytes(mul(r_inv, R)), point_bytes(mul(-d * r_inv, G))


def compute_rtu(q_xy, sig, digest):
    """-> (status, r_xy, t_xy, u_xy)"""
    Q = _checked_point(q_xy)
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:64], "big")
    if Q is None or not (1 <= r < N and 1 <= s < N):
        return MALFORMED, ZERO_POINT, ZERO_POINT, ZERO_POINT
    d = int.from_bytes(digest, "big") % N
    s_inv = pow(s, -1, N)
    R = add(mul(d * s_inv, G), mul(r * s_inv, Q))
    if R is None or R[0] % N != r:
        return BAD_SIGNATURE, ZERO_POINT, ZERO_POINT, ZERO_POINT
    r_inv = pow(r, -1, N)
    return MADE, point_bytes(R), point_bytes(mul(r_inv, R)), point_bytes(mul(-d * r_inv, G))


def sign(priv, digest, k):
    """ECDSA with the nonce k: (Q, r, s), or None where k gives r = 0 or s = 0"""
    d = int.from_bytes(digest, "big") % N
    R = mul(k, G)
    if R is None:
        return None
    r = R[0] % N
    s = pow(k, -1, N) * (d + r * priv) % N
    if r == 0 or s == 0:
        return None
    return mul(priv, G), r, s


def signed_rows(seed, count):
    """`count` valid rows (q_xy, sig, digest) from a seeded generator"""
    rng = random.Random(seed)
    rows = []
    while len(rows) < count:
        priv, k = rng.randrange(1, N), rng.randrange(1, N)
        digest = bytes(rng.randrange(256) for _ in range(32))
        made = sign(priv, digest, k)
        if made:
            Q, r, s = made
            rows.append((point_bytes(Q), be(r) + be(s), digest))
    return rows


def terms_of(q_xy, sig, digest):
    """(u G, v Q) of a row's verification: the two partial sums whose coincidence a test arranges"""
    Q = _checked_point(q_xy)
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:64], "big")
    d = int.from_bytes(digest, "big") % N
    s_inv = pow(s, -1, N)
    return mul(d * s_inv, G), mul(r * s_inv, Q)


def coincident_row(priv, k, opposite=False):
    """A row (q_xy, sig, digest) whose partial sums coincide.  With R = k G, r = R.x and s = (d + r priv) / k the sums are
    u G = (d / s) G and v Q = (r priv / s) G: they are equal where d = r priv, so the digest is chosen from r, the signature
    is valid and the final sum is a doubling.  `opposite`: d = -r priv, so u G = -(v Q) and R is the identity whatever s
    is; a signer would get s = 0 there, so s is set to k and the row is no signature."""
    Q = mul(priv, G)
    r = mul(k, G)[0] % N
    d = (-r * priv if opposite else r * priv) % N
    s = k if opposite else pow(k, -1, N) * (d + r * priv) % N
    return point_bytes(Q), be(r) + be(s), be(d)
