"""A pure-Python T-256 over integers, the oracle of the T-256 tests: affine formulas and pow(x, -1, p), nothing shared with
csrc/ft256.hpp or csrc/t256.hpp.

The curve (forks/halo2curves/src/t256/curve.rs:35-59, fp.rs:10): y^2 = x^3 - 3x + b over p_T, of prime order q = P-256's base
prime.  This file asserts, when it is imported, that G is on the curve and that q·G = O.

The byte forms are halo2curves' (serde.rs:174-319, src/derive/curve.rs:69-73 and :139-181, derive/src/field/mod.rs:326-344
and :470-476), restated; the reference pins no T-256 bytes, so they are UNVERIFIED readings and each has exactly
one writer here: `compressed` and `uncompressed`.  A point is None (the identity) or (x, y).

A set of generators is g_j = k_j·G with known k_j, so that a row sum_j z_j g_j + blind h has the closed form
(sum_j z_j k_j + blind k_h mod q)·G: ONE scalar multiplication, which keeps wide rows affordable."""
import random

PT = 0xffffffff0000000100000000000000017e72b42b30e7317793135661b1c4b117
Q = 0xffffffff00000001000000000000000000000000ffffffffffffffffffffffff      # the order: P-256's base prime
A = PT - 3
B = 0xB441071B12F4A0366FB552F8E21ED4AC36B06ACEEB354224863E60F20219FC56
G = (5, 0x3E86C0CFEBF2C7165EFC7B55F6B24FBE0ED60B9E33CE397C5826108A653DE28D)

MADE, MALFORMED = 1, 2
IDENTITY_COMPRESSED = b"\x40" + bytes(32)
ZERO_ROW = bytes(33)
TOP_DIGIT = 0xFF << 248          # a single non-zero byte, the top one; below q


def on_curve(pt):
    if pt is None:
        return True
    x, y = pt
    return 0 <= x < PT and 0 <= y < PT and (y * y - (x * x * x + A * x + B)) % PT == 0


def neg(pt):
    return None if pt is None else (pt[0], (PT - pt[1]) % PT)


def add(p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if (y1 + y2) % PT == 0:
            return None
        lam = (3 * x1 * x1 + A) * pow(2 * y1, -1, PT) % PT
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, PT) % PT
    x3 = (lam * lam - x1 - x2) % PT
    return x3, (lam * (x1 - x3) - y1) % PT


def mul(k, pt):
    k %= Q
    acc = None
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt = add(pt, pt)
        k >>= 1
    return acc


assert A == PT - 3 and PT % 4 == 3 and PT > 1 << 255
assert on_curve(G)
assert mul(Q - 1, G) == neg(G) and add(mul(Q - 1, G), G) is None          # q·G = O (mul itself reduces its scalar mod q)


# ---- bytes: one writer per form ------------------------------------------------------------------------------------------------
def be(v):
    return int(v).to_bytes(32, "big")


def scalar_bytes(v):
    """a scalar: 32 bytes little-endian; any integer below 2^256, so that a test can write a non-canonical one"""
    return int(v).to_bytes(32, "little")


def uncompressed(pt):
    return bytes(64) if pt is None else be(pt[0]) + be(pt[1])


def compressed(pt):
    if pt is None:
        return IDENTITY_COMPRESSED
    return bytes([(pt[1] & 1) << 7]) + be(pt[0])


def parities(rows):
    """which values of the parity bit occur among compressed points that are neither the identity nor a zeroed row"""
    return {r[0] >> 7 for r in rows if r != IDENTITY_COMPRESSED and r != ZERO_ROW}


def assert_both_parities(rows):
    assert parities(rows) == {0, 1}, "the expected outputs show one value of the parity bit only"


# ---- generator sets and rows ------------------------------------------------------------------------------------------------------
class Gens:
    """g_j = k_j·G and h = k_h·G with known logarithms (none zero)"""

    def __init__(self, ks, kh):
        assert all(k % Q for k in ks) and kh % Q
        self.ks, self.kh = [k % Q for k in ks], kh % Q
        self.points = [mul(k, G) for k in self.ks]
        self.h = mul(self.kh, G)
        self.n = len(ks)

    @property
    def g_xy(self):
        return b"".join(uncompressed(p) for p in self.points)

    @property
    def h_xy(self):
        return uncompressed(self.h)

    def row_scalar(self, z, blind):
        return (sum(zj * kj for zj, kj in zip(z, self.ks)) + blind * self.kh) % Q

    def commit(self, z, blind):
        """(status, 33 bytes) of one row by the closed form; MALFORMED and zero bytes where a scalar or the blind is >= q"""
        assert len(z) == self.n
        if any(not 0 <= v < Q for v in z) or not 0 <= blind < Q:
            return MALFORMED, ZERO_ROW
        return MADE, compressed(mul(self.row_scalar(z, blind), G))

    def commit_term_by_term(self, z, blind):
        acc = mul(blind, self.h)
        for zj, p in zip(z, self.points):
            acc = add(acc, mul(zj, p))
        return compressed(acc)


class PointGens(Gens):
    """generators given as points, with no known logarithm (tests/t256_steer_vectors.py chooses their coordinates): a row's
    expected value is the sum term by term, a scalar multiplication per non-zero term"""

    def __init__(self, points, h):
        assert all(p is not None and on_curve(p) for p in list(points) + [h])
        self.points, self.h, self.n = list(points), h, len(points)

    def commit(self, z, blind):
        assert len(z) == self.n
        if any(not 0 <= v < Q for v in z) or not 0 <= blind < Q:
            return MALFORMED, ZERO_ROW
        return MADE, self.commit_term_by_term(z, blind)


def make_gens(seed, n):
    rng = random.Random(seed)
    return Gens([rng.randrange(1, Q) for _ in range(n)], rng.randrange(1, Q))


def factored_lens(num_vars):
    """compute_factored_lens (forks/Spartan-t256/src/dense_mlpoly.rs:88-90): (L, R)"""
    return 1 << (num_vars // 2), 1 << (num_vars - num_vars // 2)


def hyrax(gens, num_vars, vars_, blinds):
    """DensePolynomial::commit of one proof: (status, L x 33 bytes); a scalar or blind >= q makes the whole proof MALFORMED"""
    L, R = factored_lens(num_vars)
    assert gens.n == R and len(vars_) == L * R and len(blinds) == L
    rows = [gens.commit(vars_[i * R:(i + 1) * R], blinds[i]) for i in range(L)]
    if any(st != MADE for st, _ in rows):
        return MALFORMED, ZERO_ROW * L
    return MADE, b"".join(r for _, r in rows)


def mixed_scalars(rng, n):
    """a circuit's mix of wires: mostly 0 and 1, some full-width"""
    out = []
    for _ in range(n):
        u = rng.random()
        out.append(0 if u < 0.5 else 1 if u < 0.8 else rng.randrange(Q))
    return out
