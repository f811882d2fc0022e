"""Poseidon as neptune states it (ecdsa-pop/neptune), restated generically in Python integers: parameterised by the prime and
its bit length, so that the same lines that reproduce the reference's recorded answers over BLS12-381's Fr
(tests/golden/neptune_kats.json) give the constants, the permutation and h_Q over P-256's base field.  Shares no code with
the library.

Three readings that no recorded value pins, each one function here and one in csrc/poseidon_p256.hpp:
  1. first_byte_bits   the Grain draw where the field's bit length is a multiple of 8
  2. hq_sponge         the sponge sequence behind `compute_hQ`
  3. hq_bytes          the byte order of its output"""
import math

P256 = 2**256 - 2**224 + 2**192 + 2**96 - 1
BLS12_381_FR = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
BN254_FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617


# ---- round numbers (round_numbers.rs): the smallest S-box count that is secure, with the margin of +2 full rounds and +7.5 %
def _secure(t, rf, rp, n=256.0, m=128.0):
    rf_stat = 6.0 if m <= (n - 3.0) * (t + 1.0) else 10.0
    bounds = [rf_stat, 0.43 * m + math.log2(t) - rp, 0.21 * n - rp, (0.14 * n - 1.0 - rp) / (t - 1.0)]
    return rf >= max(math.ceil(x) for x in bounds)


def round_numbers(t):
    rf = rp = 0
    cost = 1 << 60
    for rf_test in range(2, 1001, 2):
        for rp_test in range(4, 200):
            if _secure(t, rf_test, rp_test):
                a, b = rf_test + 2, math.ceil(1.075 * rp_test)
                n_sbox = t * a + b
                if n_sbox < cost or (n_sbox == cost and a < rf):
                    rf, rp, cost = a, b, n_sbox
    return rf, rp


# ---- the Grain LFSR (round_constants.rs)
def first_byte_bits(field_bits):
    """reading 1"""
    return field_bits % 8 or 8


class Grain:
    def __init__(self, field_bits, t, rf, rp):
        word = lambda n, v: [(v >> i) & 1 for i in range(n - 1, -1, -1)]
        self.state = word(2, 1) + word(4, 1) + word(12, field_bits) + word(12, t) + word(10, rf) + word(10, rp) + word(30, (1 << 30) - 1)
        self.field_bits = field_bits
        for _ in range(160):
            self._step()

    def _step(self):
        s = self.state
        b = s[62] ^ s[51] ^ s[38] ^ s[23] ^ s[13] ^ s[0]
        s.pop(0)
        s.append(b)
        return b

    def _bit(self):
        first = self._step()
        while not first:
            self._step()
            first = self._step()
        return self._step()

    def _bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self._bit()
        return v

    def draw(self):
        """32 bytes big-endian, the first of them short"""
        return int.from_bytes(bytes([self._bits(first_byte_bits(self.field_bits))] + [self._bits(8) for _ in range(31)]), "big")


class Constants:
    def __init__(self, p, field_bits, t):
        self.p, self.t = p, t
        self.rf, self.rp = round_numbers(t)
        g = Grain(field_bits, t, self.rf, self.rp)
        self.rc = []
        while len(self.rc) < (self.rf + self.rp) * t:
            v = g.draw()
            if v < p:
                self.rc.append(v)
        self.mds = [[pow(i + j + t, -1, p) for j in range(t)] for i in range(t)]       # mds.rs: x_i = i, y_j = j + t


def permute(c, state):
    """the plain ("Correct") permutation"""
    p, t, st = c.p, c.t, list(state)
    assert len(st) == t
    for r in range(c.rf + c.rp):
        st = [(x + c.rc[t * r + i]) % p for i, x in enumerate(st)]
        if r < c.rf // 2 or r >= c.rf // 2 + c.rp:
            st = [pow(x, 5, p) for x in st]
        else:
            st[0] = pow(st[0], 5, p)
        st = [sum(c.mds[i][j] * st[j] for j in range(t)) % p for i in range(t)]
    return st


def io_tag(pattern, domain_separator):
    """sponge/api.rs: `IOPattern::value`; pattern: ("absorb" | "squeeze", n) pairs"""
    mod, x = 1 << 128, (1 << 128) - 159
    merged = []
    for kind, n in pattern:
        if merged and merged[-1][0] == kind:
            merged[-1][1] += n
        else:
            merged.append([kind, n])
    xi, acc = 1, 0
    for kind, n in merged:
        if n == 0:
            continue
        xi = xi * x % mod
        acc = (acc + xi * (n + (1 << 31) if kind == "absorb" else n)) % mod
    xi = xi * x % mod
    return (acc + xi * domain_separator) % mod


# ---- P-256 and h_Q
_p256 = None


def p256():
    global _p256
    if _p256 is None:
        _p256 = Constants(P256, 256, 3)
    return _p256


HQ_TAG = io_tag([("absorb", 3), ("squeeze", 1)], 0)


def hq_sponge(q0, q1, z):
    """reading 2"""
    c = p256()
    st = permute(c, [HQ_TAG, q0 % P256, q1 % P256])
    st[1] = (st[1] + z) % P256
    return permute(c, st)[1]


def hq_bytes(h):
    """reading 3"""
    return int(h).to_bytes(32, "big")


def hq(q0, q1, z):
    return hq_bytes(hq_sponge(q0, q1, z))


def table():
    """the elements a handle uploads, in the library's order: round constants, the matrix row-major, the tag"""
    c = p256()
    return c.rc + [x for row in c.mds for x in row] + [HQ_TAG]
