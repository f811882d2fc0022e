"""Inputs whose transforms are known in closed form, and circuits whose quotient vanishes: what random data never gives the
lazy 29-bit transforms (csrc/wmap29.hip) - outputs that are exactly 0 mod r (they reach the last pass as lazy multiples k·N),
butterflies with u == t, whole tiles of equal values.  tests/test_transform_values_cpu.py shows without a GPU that every
closed form here is what oracle/ and cpu_ref compute; tests/test_gpu_transform_values.py runs them on the GPU.

n = 2^logn, w = root_of_unity(n), g = 5.  A mode is (inverse, coset):
    fft          out_k = sum x_i w^(ik)              ifft          out_k = 1/n sum x_i w^(-ik)
    coset fft    out_k = sum x_i g^i w^(ik)          coset ifft    out_k = g^(-k)/n sum x_i w^(-ik)
"""
import numpy as np

import bn254_oracle as o
import cpu_ref

R = o.R
G = o.FR_GENERATOR
MODES = [(False, False), (True, False), (False, True), (True, True)]
MODE_IDS = ["fft", "ifft", "coset_fft", "coset_ifft"]
CONSTANTS = [1, R - 1, (R - 1) // 2]


def inv(x):
    return pow(x % R, R - 2, R)


def fr_bytes(x):
    return np.frombuffer(int(x % R).to_bytes(32, "little"), np.uint8)


def k0_choices(n):
    """0 (the constant vector), 1, n/2 (+-c alternating), n - 1, one odd index near n/3"""
    return sorted({0, 1 % n, n // 2, n - 1, ((n // 3) | 1) % n})


def delta_choices(n):
    return sorted({0, 1 % n, n // 2, n - 1})


def sparse(n, idx=None, value=0):
    out = np.zeros(n * 32, np.uint8)
    if idx is not None:
        out[idx * 32:(idx + 1) * 32] = fr_bytes(value)
    return out


def geometric(mode, logn, k0, c):
    """-> (input bytes, k0, the one non-zero output): every other output is exactly zero"""
    inverse, coset = mode
    n = 1 << logn
    w = o.root_of_unity(n)
    if not inverse:
        t = inv(pow(w, k0, R)) * (inv(G) if coset else 1) % R       # c (g^-1 w^-k0)^i -> n c at k0
        value = n * c % R
    else:
        t = pow(w, k0, R)                                           # c w^(k0 i) -> c at k0 (times g^-k0 on the coset)
        value = c * (inv(pow(G, k0, R)) if coset else 1) % R
    return cpu_ref.fr_powers(c, t, n), k0, value


def delta(mode, logn, j, c):
    """c e_j -> (input bytes, the dense output as ONE fr_powers call)"""
    inverse, coset = mode
    n = 1 << logn
    w = o.root_of_unity(n)
    if not inverse:
        s, t = c * (pow(G, j, R) if coset else 1) % R, pow(w, j, R)
    else:
        s, t = c * inv(n) % R, inv(pow(w, j, R)) * (inv(G) if coset else 1) % R
    return sparse(n, j, c), cpu_ref.fr_powers(s, t, n)


def families(mode, logn, constants=CONSTANTS):
    """every vector of the three families: (label, input, expected output)"""
    n = 1 << logn
    for c in constants:
        for k0 in k0_choices(n):
            x, k, v = geometric(mode, logn, k0, c)
            yield "geometric k0=%d c=%#x" % (k0, c % (1 << 16)), x, sparse(n, k, v)
        for j in delta_choices(n):
            x, e = delta(mode, logn, j, c)
            yield "delta j=%d c=%#x" % (j, c % (1 << 16)), x, e
    yield "zero", sparse(n), sparse(n)


def mismatches(got, want):
    """indices of the 32-byte elements that differ"""
    g = np.ascontiguousarray(got, np.uint8).reshape(-1, 32)
    w = np.ascontiguousarray(want, np.uint8).reshape(-1, 32)
    assert g.shape == w.shape, (g.shape, w.shape)
    return np.nonzero((g != w).any(axis=1))[0]


def report(wrong, label, got, want):
    """appends (label, count, first few (index, got, want)) when the two differ"""
    bad = mismatches(got, want)
    if bad.size:
        g, w = np.ascontiguousarray(got, np.uint8).reshape(-1, 32), np.ascontiguousarray(want, np.uint8).reshape(-1, 32)
        first = [(int(i), hex(int.from_bytes(g[i].tobytes(), "little")), hex(int.from_bytes(w[i].tobytes(), "little"))) for i in bad[:3]]
        wrong.append((label, int(bad.size), first))


# ---- circuits whose quotient vanishes -------------------------------------------------------------------------------------
class Circuit:
    """mats: three cpu_ref.Csr; w: the full assignment, M x 32 canonical bytes"""

    def __init__(self, name, mats, l, m, M, w):
        self.name, self.mats, self.l, self.m, self.M, self.w = name, mats, l, m, M, w
        self.D = 1
        while self.D < m + l:
            self.D <<= 1

    def side_values(self, k, nthreads=1):
        """<M_k row i, w> on the D points of the domain (rows m .. m+l-1 of the a side hold the instance wires)"""
        v = np.zeros((self.D, 32), np.uint8)
        v[:self.m] = cpu_ref.spmv(self.mats[k], self.m, self.M, self.w, nthreads=nthreads).reshape(self.m, 32)
        if k == 0:
            v[self.m:self.m + self.l] = self.w.reshape(self.M, 32)[:self.l]
        return v

    def coset_sides(self, nthreads=1):
        """vinv·a(g w^j) and b(g w^j), j < D, as ints (the construction of tests/test_gpu_circom_rows.py)"""
        vinv = inv(pow(G, self.D, R) - 1)
        sides = []
        for k in range(2):
            e = cpu_ref.ntt(cpu_ref.ntt(self.side_values(k, nthreads), inverse=True, nthreads=nthreads), coset=True, nthreads=nthreads)
            raw = e.tobytes()
            sides.append([int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)])
        return [x * vinv % R for x in sides[0]], sides[1]


def ints_bytes(vals):
    return np.frombuffer(b"".join(int(v % R).to_bytes(32, "little") for v in vals), np.uint8).copy()


def _random_fr(rng, n):
    x = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    x[:, 31] &= 0x1f                                     # below 2^253 < r
    return x


def _single_column(m, col, coeff_rows):
    return cpu_ref.Csr(np.arange(m + 1, dtype=np.uint64), np.full(m, col, np.uint32), np.ascontiguousarray(coeff_rows).reshape(-1))


def b_and_c_vanish(D, seed=1, l=2, M=48):
    """Ordinary random A rows (three terms each); every B row one term on a wire that is 0, every C row likewise on another.
    b = c = 0 on the whole domain, so h = 0 and q_j = 0 at every index while a is dense and non-zero."""
    rng = np.random.default_rng(seed)
    m = D - l - 3                                        # no multiple of anything; rows m+l .. D-1 are padding
    pool = _random_fr(rng, 1024)
    pool[0] = 0
    pool[0, 0] = 1                                       # the literal one takes the product-free path of the sparse product
    A = cpu_ref.Csr(np.arange(m + 1, dtype=np.uint64) * 3, rng.integers(0, M - 2, size=3 * m).astype(np.uint32),
                    pool[rng.integers(0, 1024, size=3 * m)].reshape(-1))
    B = _single_column(m, M - 1, pool[rng.integers(0, 1024, size=m)])
    C = _single_column(m, M - 2, pool[rng.integers(0, 1024, size=m)])
    w = _random_fr(rng, M)
    w[0] = 0
    w[0, 0] = 1
    w[M - 1] = 0
    w[M - 2] = 0
    return Circuit("b_and_c_vanish", (A, B, C), l, m, M, w.reshape(-1))


def constant_sides(D, beta, seed=2, M=8):
    """l = 1, m = D - 1; every A row 1·w0, every B row beta·w0, every C row beta·w0.  a = 1 on all D points (row m holds the
    instance wire w0 = 1), b = c as polynomials, so a·b - c = 0 identically and h = 0; q_j = vinv·b(g w^j) is dense."""
    rng = np.random.default_rng(seed)
    l, m = 1, D - 1
    one = np.zeros((1, 32), np.uint8)
    one[0, 0] = 1
    bb = fr_bytes(beta).reshape(1, 32)
    A = _single_column(m, 0, np.repeat(one, m, axis=0))
    B = _single_column(m, 0, np.repeat(bb, m, axis=0))
    C = _single_column(m, 0, np.repeat(bb, m, axis=0))
    w = _random_fr(rng, M)
    w[0] = one[0]
    return Circuit("constant_sides", (A, B, C), l, m, M, w.reshape(-1))
