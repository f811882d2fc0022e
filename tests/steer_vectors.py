"""Inputs steered to the rare branch of csrc/fp256.hpp and csrc/fq256.hpp, and to the cases of `compute_TU` and `compute_RTU`
that pseudo-random rows never meet.  Pure Python integers; shares no code with the library.  Expected bytes and statuses are
the oracles' (tests/p256_vectors.py, tests/poseidon_vectors.py), never this file's.

The rare branch.  Both moduli m are about 2^256 - 2^224, and after every sum and every product `reduce_once` takes one of
three cases: a ninth bit, no ninth bit and eight words below m, or - with probability about 2^-32 on random operands - no
ninth bit and eight words NOT below m.  The integer model of the last one:

    mont(v, m)   = v 2^256 mod m                                 the representation of the value v
    pre(a, b, m) = (a b + ((-a b m^-1) mod 2^256) m) >> 256      what a word-by-word Montgomery product of the representations
                                                                 a and b holds before its conditional subtraction, whatever
                                                                 the word size
    a product hits the branch   iff m <= pre(a, b, m) < 2^256
    a sum of A and B hits it    iff m <= A + B < 2^256
    from_words(x) is the product of x with 2^512 mod m

A product whose result has a small representation rho hits it almost always: pre is rho or rho + m, and it is rho only where
a b <= rho 2^256.  So a site is steered by choosing the VALUE it computes as rho 2^-256 and solving for the input.

Every vector is found by a seeded, bounded search and carries the facts a test needs to show, with the model above, that it
hits the case it is named for (tests/test_steer_vectors_cpu.py); an exhausted search raises."""
import collections
import functools
import random

import p256_vectors as V
import poseidon_vectors as PV

P, N, G, B = V.P, V.N, V.G, V.B
R = 1 << 256
FR = PV.BN254_FR
MADE, MALFORMED, BAD_SIGNATURE = V.MADE, V.MALFORMED, V.BAD_SIGNATURE
ZERO_WINDOWS = (0xAB << 248) | (0x0F << 120) | 0x10      # tests/test_p256_host.py's: most 8-bit and 4-bit windows are zero
ONES = int("01" * 32, 16)
DELTA_MAX = R - 1 - P                                    # 2^224 - 2^192 - 2^96: p + DELTA_MAX = 2^256 - 1
_MINV = {m: pow(m, -1, R) for m in (P, N)}
_RINV = {m: pow(R, -1, m) for m in (P, N)}
TRIES = 4000


# ---- the integer model ---------------------------------------------------------------------------------------------------------
def mont(v, m):
    return v * R % m


def unmont(rep, m):
    return rep * _RINV[m] % m


def pre(a, b, m):
    t = a * b
    return (t + (-t * _MINV[m]) % R * m) >> 256


def rare(value, m):
    return m <= value < R


def mul_hits(a, b, m):
    """a, b: representations"""
    return rare(pre(a, b, m), m)


def add_hits(a, b, m):
    return rare(a + b, m)


def from_words_hits(x, m):
    """x: canonical words, below m"""
    return mul_hits(x, R * R % m, m)


def reduced_from_words_hits(x, m):
    """q256_from_words_reduced: any 256-bit x, reduced once, then taken into Montgomery form"""
    return from_words_hits(x - m if x >= m else x, m)


# ---- P-256: points and the two constructions -------------------------------------------------------------------------------------
def sqrt_p(t):
    r = pow(t, (P + 1) // 4, P)                          # p = 3 mod 4
    return r if r * r % P == t % P else None


def lift_x(x, odd=0):
    """the point (x, y) with y of the given parity, or None"""
    y = sqrt_p((x * x * x - 3 * x + B) % P)
    if y is None or x >= P:
        return None
    return (x, y if y & 1 == odd else P - y)


def _strip(a):
    while a and a[-1] == 0:
        a.pop()
    return a


def _poly_mod(a, f):
    a = [c % P for c in a]
    _strip(a)
    lead = pow(f[-1], -1, P)
    while len(a) >= len(f):
        c, at = a[-1] * lead % P, len(a) - len(f)
        for i, fi in enumerate(f):
            a[at + i] = (a[at + i] - c * fi) % P
        _strip(a)
    return a


def _poly_mulmod(a, b, f):
    out = [0] * (len(a) + len(b) - 1) if a and b else []
    for i, ai in enumerate(a):
        for j, bj in enumerate(b):
            out[i + j] += ai * bj
    return _poly_mod(out, f)


def x_of_y(y):
    """the x with (x, y) on the curve where x^3 - 3x + b - y^2 has exactly one root in the field (half of all y), else None:
    that root is gcd(x^p - x, cubic)"""
    f = [(B - y * y) % P, P - 3, 0, 1]
    acc = [1]
    for bit in bin(P)[2:]:
        acc = _poly_mulmod(acc, acc, f)
        if bit == "1":
            acc = _poly_mulmod(acc, [0, 1], f)
    g = acc + [0] * max(0, 2 - len(acc))
    g[1] = (g[1] - 1) % P
    a, b = f, _strip(g)
    while b:
        a, b = b, _poly_mod(a, b)
    if len(a) != 2:
        return None
    x = -a[0] * pow(a[1], -1, P) % P
    assert V.on_curve((x, y))
    return x


def rand_point(rng):
    while True:
        pt = lift_x(rng.randrange(P), rng.randrange(2))
        if pt:
            return pt


def forged_r(X, u, v, digest=None):
    """A valid row (q_xy, sig, digest) of compute_RTU whose R is the chosen on-curve X, without a discrete logarithm:
    r = X.x mod n, s = r / v, d = u s and Q = v^-1 (X - u G), so that u G + v Q = X.  `digest`: other bytes that are d mod n."""
    r = X[0] % N
    s = r * pow(v, -1, N) % N
    d = u * s % N
    Q = V.mul(pow(v, -1, N), V.add(X, V.neg(V.mul(u, G))))
    assert r and s and Q is not None
    digest = V.be(d) if digest is None else digest
    assert int.from_bytes(digest, "big") % N == d
    return V.point_bytes(Q), V.be(r) + V.be(s), digest


def free_q(Q, u, v):
    """A valid row on the chosen on-curve Q: R = u G + v Q, r = R.x mod n, s = r / v, d = u s"""
    Rpt = V.add(V.mul(u, G), V.mul(v, Q))
    r = Rpt[0] % N
    s = r * pow(v, -1, N) % N
    assert r and s
    return V.point_bytes(Q), V.be(r) + V.be(s), V.be(u * s % N)


def rtu_scalars(q_xy, sig, digest):
    """the five scalars of a compute_RTU row in the library's order: the chains (r/s) Q and (1/s) Q, then the walks (d/s) G,
    (d/(r s)) G and (-d/r) G.  For the two constructions: v, v/r, u, u/r, -d/r."""
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    d = int.from_bytes(digest, "big") % N
    si, ri = pow(s, -1, N), pow(r, -1, N)
    return [r * si % N, si, d * si % N, d * si * ri % N, -d * ri % N]


def tu_scalars(r_xy, digest):
    """the chain scalar r^-1 on R and the walk scalar -d/r of a compute_TU row"""
    ri = pow(int.from_bytes(r_xy[:32], "big") % N, -1, N)
    return [ri, -int.from_bytes(digest, "big") * ri % N]


# kind: "tu" with args (r_xy, digest) or "rtu" with args (q_xy, sig, digest); status: what the construction promises;
# facts: what the CPU test feeds the model
Vec = collections.namedtuple("Vec", "name kind args status facts")


@functools.lru_cache(maxsize=None)
def expected(vec):
    """the oracle's answer: (status, t, u) or (status, r, t, u)"""
    return V.compute_tu(*vec.args) if vec.kind == "tu" else V.compute_rtu(*vec.args)


def _vec(name, kind, args, status=MADE, **facts):
    return Vec(name, kind, tuple(args), status, tuple(sorted(facts.items())))


def facts(vec):
    return dict(vec.facts)


def _digest(rng):
    return bytes(rng.randrange(256) for _ in range(32))


def _signed(rng, digest):
    while True:
        made = V.sign(rng.randrange(1, N), digest, rng.randrange(1, N))
        if made:
            Q, r, s = made
            return V.point_bytes(Q), V.be(r) + V.be(s), digest


def family_rx_above_n():
    """1. R.x in [n, p): the reduction of R.x in both calls"""
    rng = random.Random(0x57EE1)
    out = []
    for j in (3, 4, 6, 9):
        X = lift_x(N + j, j & 1)
        if X is None:
            raise RuntimeError("n + %d is no x-coordinate" % j)
        out.append(_vec("tu x=n+%d" % j, "tu", (V.point_bytes(X), _digest(rng)), X=X))
        for u, v in ((0x77, 0x99), (0, 5), (1, 1), (N - 1, N - 1)):
            q, sig, dg = forged_r(X, u, v)
            tag = "x=n+%d u=%x v=%x" % (j, u, v)
            out.append(_vec("rtu " + tag, "rtu", (q, sig, dg), X=X, u=u, v=v))
            out.append(_vec("rtu r unreduced " + tag, "rtu", (q, V.be(X[0]) + sig[32:], dg), MALFORMED, X=X))
            out.append(_vec("rtu r+1 " + tag, "rtu", (q, V.be(X[0] - N + 1) + sig[32:], dg), BAD_SIGNATURE, X=X))
    return out


def family_digests():
    """2. digests = 0 mod n and >= n in compute_RTU, and compute_TU on each R it returns"""
    rng = random.Random(0x57EE2)
    rows = []
    for value in (0, N):
        rows.append(("forged digest=%x" % value, forged_r(rand_point(rng), 0, rng.randrange(1, N), digest=V.be(value))))
        rows.append(("signed digest=%x" % value, _signed(rng, V.be(value))))
    for value in (N + 5, R - 1):
        rows.append(("signed digest=%x" % value, _signed(rng, V.be(value))))
    out = []
    for name, row in rows:
        out.append(_vec("rtu " + name, "rtu", row, digest=int.from_bytes(row[2], "big")))
        out.append(_vec("tu " + name, "tu", (V.compute_rtu(*row)[1], row[2]), digest=int.from_bytes(row[2], "big")))
    return out


WALK_SCALARS = (1, 2, 255, 256, 1 << 248, 255 << 248, N - 1, N - 2, ZERO_WINDOWS, ONES)
CHAIN_SCALARS = (1, 2, 15, 16, 17, 1 << 252, 15 << 252, N - 1, ZERO_WINDOWS % N)


def family_structured_scalars():
    """3. scalars with structure in the table walk (compute_TU's U = k G with d = -k r) and in the windowed chain (forged-R
    rows whose first chain scalar is v, then rows whose second, 1/s = v/r, is c)"""
    rng = random.Random(0x57EE3)
    out = []
    for k in WALK_SCALARS:
        Rpt = rand_point(rng)
        d = -k * (Rpt[0] % N) % N
        out.append(_vec("walk k=%x" % k, "tu", (V.point_bytes(Rpt), V.be(d)), term=1, scalar=k))
    for c in CHAIN_SCALARS:
        X = rand_point(rng)
        out.append(_vec("chain v=%x" % c, "rtu", forged_r(X, rng.randrange(1, N), c), term=0, scalar=c))
        X = rand_point(rng)
        out.append(_vec("chain 1/s=%x" % c, "rtu", forged_r(X, rng.randrange(1, N), c * (X[0] % N) % N), term=1, scalar=c))
    return out


def _search(rng, make):
    for _ in range(TRIES):
        got = make(rng)
        if got is not None:
            return got
    raise RuntimeError("search bound exhausted")


def _point_x_hits(rng):
    pt = lift_x(unmont(rng.randrange(1, 4000), P), rng.randrange(2))
    return pt if pt and from_words_hits(pt[0], P) else None


def _point_y_hits(rng):
    y = unmont(rng.randrange(1, 1 << 200), P)
    x = x_of_y(y)
    return (x, y) if x is not None and from_words_hits(y, P) else None


def _point_with_mont_x_in(lo, hi):
    def make(rng):
        return lift_x(unmont(rng.randrange(lo, hi), P), rng.randrange(2))
    return make


def coordinate_sites(pt):
    """which of the entry-point sites of p256_read_point and p256_on_curve the point hits, by the model"""
    m = mont(pt[0], P)
    hit = set()
    if from_words_hits(pt[0], P):
        hit.add("x from_words")
    if from_words_hits(pt[1], P):
        hit.add("y from_words")
    if add_hits(m, m, P):
        hit.add("x + x")
    if add_hits(2 * m % P, m, P):
        hit.add("2x + x, 2m < p" if 2 * m < P else "2x + x, 2m >= p")
    return hit


def family_entry_points():
    """4. the field entry points at the rare branch: coordinates (each point as R of compute_TU and as Q of a free-Q row of
    compute_RTU) and the scalars d, s and r"""
    rng = random.Random(0x57EE4)
    third = lambda v: -(-v // 3)
    makers = (("x from_words", _point_x_hits), ("y from_words", _point_y_hits),
              ("x + x", _point_with_mont_x_in(-(-P // 2), 1 << 255)),
              ("2x + x, 2m < p", _point_with_mont_x_in(third(P), third(R))),
              ("2x + x, 2m >= p", _point_with_mont_x_in(third(2 * P), third(R + P))))
    out = []
    for site, make in makers:
        for i in range(2):
            pt = _search(rng, make)
            out.append(_vec("tu R: %s #%d" % (site, i), "tu", (V.point_bytes(pt), _digest(rng)), point=pt, site=site))
            out.append(_vec("rtu Q: %s #%d" % (site, i), "rtu", free_q(pt, rng.randrange(1, N), rng.randrange(1, N)), point=pt, site=site))
    for i in range(2):
        d = _search(rng, lambda g: (lambda x: x if from_words_hits(x, N) else None)(unmont(g.randrange(1, 1 << 200), N)))
        row = _signed(rng, V.be(d))
        out.append(_vec("rtu d to_mont #%d" % i, "rtu", row, site="d", scalar=d))
        out.append(_vec("tu d to_mont #%d" % i, "tu", (V.compute_rtu(*row)[1], row[2]), site="d", scalar=d))
        s = _search(rng, lambda g: (lambda x: x if from_words_hits(x, N) else None)(unmont(g.randrange(1, 1 << 200), N)))
        X = rand_point(rng)
        out.append(_vec("rtu s to_mont #%d" % i, "rtu", forged_r(X, rng.randrange(1, N), (X[0] % N) * pow(s, -1, N) % N), site="s", scalar=s))

        def r_hits(g):
            x = unmont(g.randrange(1, 1 << 200), N)
            pt = lift_x(x, g.randrange(2))
            return pt if pt and from_words_hits(x, N) else None
        X = _search(rng, r_hits)
        out.append(_vec("rtu r to_mont #%d" % i, "rtu", forged_r(X, rng.randrange(1, N), rng.randrange(1, N)), site="r", scalar=X[0]))
        out.append(_vec("tu r to_mont #%d" % i, "tu", (V.point_bytes(X), _digest(rng)), site="r", scalar=X[0]))
    return out


P256_FAMILIES = (("rx_above_n", family_rx_above_n), ("digests", family_digests), ("structured_scalars", family_structured_scalars),
                 ("entry_points", family_entry_points))
P256_COUNTS = {"rx_above_n": 4 + 3 * 16, "digests": 12, "structured_scalars": 10 + 18, "entry_points": 20 + 10}


@functools.lru_cache(maxsize=None)
def p256_families():
    """family name -> its vectors, built once per process"""
    return {name: tuple(make()) for name, make in P256_FAMILIES}


# ---- Poseidon over P-256's base field: round 0 ---------------------------------------------------------------------------------------
# 25 divides p - 1 (and 125 does not), so x^5 is no bijection and a later round's state cannot be inverted to an input; but the
# device's round loop is rolled, and round 0 is a full round: it runs every add and product site of every later one.
# T is a fifth power iff T^((p-1)/5) = 1.  With p - 1 = 25 m: T^(1/5 mod m) is a fifth root of T up to a fifth root of unity,
# which one of the 25th roots of unity puts right.
M25 = (P - 1) // 25
E5 = pow(5, -1, M25)
W25 = next(pow(h, M25, P) for h in range(2, 100) if pow(h, (P - 1) // 5, P) != 1)      # of order 25


def is_fifth_power(t):
    return t % P == 0 or pow(t, (P - 1) // 5, P) == 1


def fifth_root(t):
    r = pow(t, E5, P)
    for _ in range(25):
        if pow(r, 5, P) == t % P:
            return r
        r = r * W25 % P
    raise ValueError("not a fifth power")


def round0_sites(state):
    """site -> the integer the model says the site holds before its conditional subtraction, for pos_permute's round 0 on the
    canonical state (three values).  Sites: ("add_rc", i), ("sqr", i), ("sqr_sqr", i), ("mul_a4_a", i), ("mds_mul", 3 i + j),
    ("mds_add", i, 0 | 1)."""
    c = PV.p256()
    sites = {}
    post = []
    for i in range(3):
        sites[("add_rc", i)] = mont(state[i], P) + mont(c.rc[i], P)
        a = (state[i] + c.rc[i]) % P
        a1, a2, a4 = mont(a, P), mont(a * a, P), mont(pow(a, 4, P), P)
        sites[("sqr", i)] = pre(a1, a1, P)
        sites[("sqr_sqr", i)] = pre(a2, a2, P)
        sites[("mul_a4_a", i)] = pre(a4, a1, P)
        post.append(pow(a, 5, P))
    for i in range(3):
        t = [mont(c.mds[i][j] * post[j], P) for j in range(3)]
        for j in range(3):
            sites[("mds_mul", 3 * i + j)] = pre(mont(c.mds[i][j], P), mont(post[j], P), P)
        sites[("mds_add", i, 0)] = t[0] + t[1]
        sites[("mds_add", i, 1)] = (t[0] + t[1]) % P + t[2]
    return sites


PVec = collections.namedtuple("PVec", "name site state")     # site: the key of round0_sites this state hits
HVec = collections.namedtuple("HVec", "name sites q")        # sites: of "q0", "q1", "z"; q: (q0, q1, z)


def _state_with(rng, fixed):
    """fixed: lane -> the S-box INPUT a of that lane; the other lanes are random"""
    c = PV.p256()
    return tuple((fixed[i] - c.rc[i]) % P if i in fixed else rng.randrange(P) for i in range(3))


def _small(rng):
    return unmont(rng.randrange(1, 1 << 200), P)


def _root4(t):
    s = sqrt_p(t)
    if s is None:
        return None
    return sqrt_p(s) or sqrt_p(P - s)


def _find_state(rng, site, build):
    """`build(rng)` -> a state or None; accepted where the model says it hits `site`"""
    def make(g):
        st = build(g)
        return st if st is not None and rare(round0_sites(st)[site], P) else None
    return _search(rng, make)


def poseidon_add_rc():
    rng = random.Random(0x905E1)
    c = PV.p256()
    out = []
    for i in range(3):
        for delta in (0, 1, DELTA_MAX):
            st = [rng.randrange(P) for _ in range(3)]
            st[i] = (unmont(delta, P) - c.rc[i]) % P
            out.append(PVec("state_%d + rc_%d = p + %x" % (i, i, delta), ("add_rc", i), tuple(st)))
    return out


def poseidon_pow5():
    rng = random.Random(0x905E2)
    roots = (("sqr", sqrt_p), ("sqr_sqr", _root4), ("mul_a4_a", lambda t: fifth_root(t) if is_fifth_power(t) else None))
    out = []
    for kind, root in roots:
        for i in range(3):
            def build(g, i=i, root=root):
                a = root(_small(g))
                return None if a is None else _state_with(g, {i: a})
            out.append(PVec("%s lane %d" % (kind, i), (kind, i), _find_state(rng, (kind, i), build)))
    return out


def mds_mul_reachable(i, j):
    """Whether the product m[3 i + j] * s can take the rare branch for ANY s.  The matrix entry is 1 / k with k = i + j + 3, its
    representation a has a k = (2^256 - p) + c p for a c in [0, k).  If the product held p + t, 0 <= t < 2^256 - p, before its
    subtraction, the other operand would be b = t k (it is t k mod p, and t k < p), so a b = t (2^256 - p) + t c p, and the
    quotient q with a b + q p = (p + t) 2^256 would be 2^256 - t (c - 1): below 2^256, as a quotient is, only where c >= 2.
    For k = 3 and 5 c is 0, for k = 4 it is 1: six of the nine products never take the branch; k = 6 and 7 can."""
    k = i + j + 3
    c, rest = divmod(k * mont(PV.p256().mds[i][j], P) - (R - P), P)
    assert rest == 0 and 0 <= c < k
    return c >= 2


def poseidon_mds_mul():
    """the three products of the matrix that can take the branch: the post-S-box value is rho 2^-256 k, a fifth power for
    one rho in five"""
    rng = random.Random(0x905E3)
    c = PV.p256()
    out = []
    for i in range(3):
        for j in range(3):
            if not mds_mul_reachable(i, j):
                continue

            def build(g, i=i, j=j):
                s = _small(g) * pow(c.mds[i][j], -1, P) % P
                return _state_with(g, {j: fifth_root(s)}) if is_fifth_power(s) else None
            out.append(PVec("m[%d] s%d" % (3 * i + j, j), ("mds_mul", 3 * i + j), _find_state(rng, ("mds_mul", 3 * i + j), build)))
    return out


def poseidon_mds_add():
    rng = random.Random(0x905E4)
    c = PV.p256()
    out = []
    for i in range(3):
        for which in (0, 1):
            def build(g, i=i, which=which):
                a = [g.randrange(P) for _ in range(3)]
                t = [mont(c.mds[i][j] * pow(a[j], 5, P), P) for j in range(3)]
                have = t[0] if which == 0 else (t[0] + t[1]) % P
                solve = 1 + which                                      # the lane solved for
                delta = g.randrange(min(have, DELTA_MAX + 1))
                s = unmont(P + delta - have, P) * pow(c.mds[i][solve], -1, P) % P
                if not is_fifth_power(s):
                    return None
                a[solve] = fifth_root(s)
                return _state_with(g, dict(enumerate(a)))
            site = ("mds_add", i, which)
            out.append(PVec("row %d add %d" % (i, which), site, _find_state(rng, site, build)))
    return out


POSEIDON_FAMILIES = (("add_rc", poseidon_add_rc), ("pow5", poseidon_pow5), ("mds_mul", poseidon_mds_mul), ("mds_add", poseidon_mds_add))
POSEIDON_COUNTS = {"add_rc": 9, "pow5": 9, "mds_mul": 3, "mds_add": 6, "hq": 6}


@functools.lru_cache(maxsize=None)
def poseidon_families():
    return {name: tuple(make()) for name, make in POSEIDON_FAMILIES}


def hq_sites(q0, q1, z):
    """which of cg_hq_batch's entry sites the triple hits: f256_from_words of q0 and of q1, and s1 + from_words(z) in front
    of the second permutation"""
    hit = set()
    if from_words_hits(q0, P):
        hit.add("q0")
    if from_words_hits(q1, P):
        hit.add("q1")
    s1 = PV.permute(PV.p256(), [PV.HQ_TAG, q0, q1])[1]
    if add_hits(mont(s1, P), mont(z, P), P):
        hit.add("z")
    return hit


@functools.lru_cache(maxsize=None)
def hq_vectors():
    rng = random.Random(0x905E5)

    def q_hits(g):
        q = unmont(g.randrange(1, 1 << 223), P)
        return q if q < FR and from_words_hits(q, P) else None

    def z_for(q0, q1):
        s1 = mont(PV.permute(PV.p256(), [PV.HQ_TAG, q0, q1])[1], P)

        def make(g):
            z = unmont(P + g.randrange(min(s1, DELTA_MAX + 1)) - s1, P)
            return z if z < FR and add_hits(s1, mont(z, P), P) else None
        return _search(rng, make)
    rand = lambda: rng.randrange(FR)
    out = []
    for sites in (("q0",), ("q1",), ("q0", "q1"), ("z",), ("z",), ("q0", "q1", "z")):
        q0 = _search(rng, q_hits) if "q0" in sites else rand()
        q1 = _search(rng, q_hits) if "q1" in sites else rand()
        z = z_for(q0, q1) if "z" in sites else rand()
        out.append(HVec("hq " + " ".join(sites), sites, (q0, q1, z)))
    return tuple(out)
