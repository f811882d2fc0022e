"""Generators and rows steered to the rare case of csrc/ft256.hpp's `ft256_reduce_once` INSIDE the kernels of
csrc/t256commit.hip: tests/steer_vectors.py's method restated for p_T.  Pure Python integers; shares no code with the library.
Expected bytes and statuses are the oracle's (tests/t256_vectors.py: `PointGens.commit`, the sum term by term), never this file's.

The rare case.  p_T is about 2^256 - 2^224, and after every sum and every product `ft256_reduce_once` takes one of three cases:
a ninth bit, no ninth bit and eight words below p_T, or - about once in 2^32 on random operands - no ninth bit and eight words
NOT below p_T.  The integer model of the last one, as tests/test_t256_host.py states it:

    mont(v)   = v 2^256 mod p_T                                     the representation of the value v
    pre(a, b) = (a b + ((-a b p_T^-1) mod 2^256) p_T) >> 256         what a word-by-word Montgomery product of the representations
                                                                    a and b holds before its conditional subtraction
    a product hits the case   iff p_T <= pre(a, b) < 2^256
    a sum of A and B hits it  iff p_T <= A + B < 2^256

A product whose result has a small representation rho hits it almost always: pre is rho or rho + p_T, and rho only where
a b <= rho 2^256.  So a site is steered by choosing the VALUE it computes as rho 2^-256 and solving for a coordinate of a
generator: the caller chooses the generators, and a generator's coordinates enter the first mixed addition of a row as they are.

The trace model (`trace_row`) restates, over canonical representations, the order of operations a row takes on the device:
`t256_walk_share` for each of the W lanes with a `t256_add_mixed` per non-zero digit in the lane's digit order, the butterfly
(s = W/2 .. 1, lane t takes `t256_add(acc_t, acc_{t+s})`), and `k_t256_finish` (the 512 steps of `ft256_inv`, the two
products with Z^-1, the two `ft256_from_mont`).  It notes every sum and every product that lands in [p_T, 2^256) before its
subtraction, as (stage, operation, where).  It decides only THAT a row hits a site, never a byte; tests/test_t256_steer_cpu.py
holds its final point against the oracle's for every vector.

What a lone generator leaves.  Every family here runs at W = 4 (two or three generators and the blind).  From the identity
(0 : 1 : 0) the mixed addition of (x, y) leaves (x y : y^2 : y), and the complete addition of (X : Y : Z) and the identity
leaves (X Y : Y^2 : Z Y).  So the partial of a lane that added one table entry (x, y) is (x y : y^2 : y), after one butterfly
step against an empty lane (x y^3 : y^4 : y^3), after two (x y^7 : y^8 : y^7).  3 and 7 divide p_T - 1, so a third or a
seventh root exists for one value in three or seven (`kth_root`).

Every vector is found by a seeded search of at most TRIES tries and accepted only where the trace model shows the hit; an
exhausted search raises."""
import collections
import functools
import random

import t256_vectors as V

PT, Q, G, B = V.PT, V.Q, V.G, V.B
R = 1 << 256
R2 = R * R % PT
DELTA_MAX = R - 1 - PT                                   # p_T + DELTA_MAX = 2^256 - 1
TRIES = 4000
_PINV, _RINV = pow(PT, -1, R), pow(R, -1, PT)
H = V.mul(0x7256B11D, G)                                 # the blind's generator of every family; no row here has a blind on a steered site


# ---- the integer model ---------------------------------------------------------------------------------------------------------
def mont(v):
    return v * R % PT


def unmont(rep):
    return rep * _RINV % PT


def pre(a, b):
    t = a * b
    return (t + (-t * _PINV) % R * PT) >> 256


def rare(value):
    return PT <= value < R


def from_mont_reachable():
    """Whether `ft256_from_mont`, the product of a representation a < p_T with the integer 1, can take the rare case for ANY a.
    It holds (a + m p_T) / 2^256 before its subtraction, with a quotient m < 2^256: less than (p_T + (2^256 - 1) p_T) / 2^256 =
    p_T.  It cannot, on any input; tests/test_t256_steer_cpu.py asserts the bound at the ends of the range and on seeded a."""
    return (PT - 1 + (R - 1) * PT) >> 256 >= PT


# ---- T-256: points with a chosen coordinate ---------------------------------------------------------------------------------------
def sqrt_pt(t):
    r = pow(t, (PT + 1) // 4, PT)                        # p_T = 3 mod 4
    return r if r * r % PT == t % PT else None


def kth_root(v, k):
    """a k-th root of v for a prime k that divides p_T - 1 = k^e m (27 and 7 do, 81 and 49 do not), or None where v has none:
    v^(1/k mod m) is a root up to an element of the subgroup of order k^e, which one of its k^e elements puts right"""
    e, m = 0, PT - 1
    while m % k == 0:
        e, m = e + 1, m // k
    assert e and k ** e <= 49
    if pow(v, (PT - 1) // k, PT) != 1:
        return None
    r = pow(v, pow(k, -1, m), PT)
    w = next(pow(h, m, PT) for h in range(2, 100) if pow(h, (PT - 1) // k, PT) != 1)     # of order k^e
    for _ in range(k ** e):
        if pow(r, k, PT) == v % PT:
            return r
        r = r * w % PT
    raise ValueError("not a k-th power")


def lift_x(x, odd=0):
    """the point (x, y) with y of the given parity, or None"""
    y = sqrt_pt((x * x * x - 3 * x + B) % PT)
    if y is None or x >= PT:
        return None
    return (x, y if y & 1 == odd else PT - y)


def _strip(a):
    while a and a[-1] == 0:
        a.pop()
    return a


def _poly_mod(a, f):
    a = [c % PT for c in a]
    _strip(a)
    lead = pow(f[-1], -1, PT)
    while len(a) >= len(f):
        c, at = a[-1] * lead % PT, len(a) - len(f)
        for i, fi in enumerate(f):
            a[at + i] = (a[at + i] - c * fi) % PT
        _strip(a)
    return a


def _poly_mulmod(a, b, f):
    out = [0] * (len(a) + len(b) - 1) if a and b else []
    for i, ai in enumerate(a):
        for j, bj in enumerate(b):
            out[i + j] += ai * bj
    return _poly_mod(out, f)


def _split_gcd(f):
    """gcd(x^p - x, f) for a monic cubic f (coefficients from the constant up): the product of f's linear factors"""
    f = [c % PT for c in f]
    acc = [1]
    for bit in bin(PT)[2:]:
        acc = _poly_mulmod(acc, acc, f)
        if bit == "1":
            acc = _poly_mulmod(acc, [0, 1], f)
    g = acc + [0] * max(0, 2 - len(acc))
    g[1] = (g[1] - 1) % PT
    a, b = f, _strip(g)
    while b:
        a, b = b, _poly_mod(a, b)
    return a


def single_root(f):
    """the root of the monic cubic f where it has exactly one in the field (half of all cubics), else None"""
    a = _split_gcd(f)
    return -a[0] * pow(a[1], -1, PT) % PT if len(a) == 2 else None


def least_root(f):
    """the least root of the monic cubic f, or None where it has none: a cubic that splits is cut by
    gcd((x + s)^((p-1)/2) - 1, .) for s = 1, 2, .. until a linear factor falls out"""
    a = _split_gcd(f)
    if len(a) == 1:
        return None
    found, todo, s = [], [a], 0
    while todo:
        a = todo.pop()
        if len(a) == 2:
            found.append(-a[0] * pow(a[1], -1, PT) % PT)
            continue
        while True:
            s += 1
            acc = [1]
            for bit in bin((PT - 1) // 2)[2:]:
                acc = _poly_mulmod(acc, acc, a)
                if bit == "1":
                    acc = _poly_mulmod(acc, [s, 1], a)
            g = acc + [0] * max(0, 1 - len(acc))
            g[0] = (g[0] - 1) % PT
            h, b = a, _strip(g)
            while b:
                h, b = b, _poly_mod(h, b)
            if 1 < len(h) < len(a):
                quotient, rest = [], list(a)
                lead = pow(h[-1], -1, PT)
                while len(rest) >= len(h):
                    c = rest[-1] * lead % PT
                    quotient.insert(0, c)
                    for i, hi in enumerate(h):
                        rest[len(rest) - len(h) + i] = (rest[len(rest) - len(h) + i] - c * hi) % PT
                    rest.pop()
                assert not _strip(rest)
                todo += [h, quotient]
                break
    return min(found)


def x_of_y(y):
    """the x with (x, y) on the curve where x^3 - 3x + b - y^2 has exactly one root, else None"""
    x = single_root([B - y * y, -3, 0, 1])
    assert x is None or V.on_curve((x, y))
    return x


def on_line(c):
    """the point (x, c - x) with the least x in which the line x + y = c meets the curve, else None: (c - x)^2 = x^3 - 3x + b
    is the cubic x^3 - x^2 + (2c - 3) x + b - c^2"""
    x = least_root([B - c * c, 2 * c - 3, -1, 1])
    if x is None:
        return None
    assert V.on_curve((x, (c - x) % PT))
    return x, (c - x) % PT


# ---- the trace model ---------------------------------------------------------------------------------------------------------------
CB, ONE = mont(B), mont(1)
IDENTITY = (0, ONE, 0)


class Trace:
    """csrc/ft256.hpp's sums, differences and products over eight-word values; `hits` collects (stage, operation, where) of
    the sums and products that hold a value in [p_T, 2^256) before the subtraction.  `ops` counts all of them.  With
    `missed` the subtraction is left out in exactly that case, as a library that lacked it would: the value stays in
    [p_T, 2^256), and the operations after it run on it word for word."""

    def __init__(self, missed=False):
        self.hits, self.ops, self.stage, self.where, self.missed = [], 0, "", None, missed

    def _note(self, value, op):
        self.ops += 1
        if rare(value):
            self.hits.append((self.stage, op, self.where))
            return value if self.missed else value - PT
        return value - PT if value >= R else value           # a ninth bit, or below p_T already

    def add(self, a, b, op):
        return self._note(a + b, op)

    def mul(self, a, b, op):
        return self._note(pre(a, b), op)

    @staticmethod
    def sub(a, b):
        """ft256_sub has no reduce_once: the difference of the words, and p_T added back after a borrow"""
        return (a - b) % R if a >= b else (a - b + PT) % R

    def triple(self, a, op):
        return self.add(self.add(a, a, op + ": a+a"), a, op + ": 2a+a")


def _add_tail(tr, xx, yy, zz, xy, xz, yz):
    A = tr.triple(tr.sub(tr.mul(CB, zz, "b·zz"), xz), "A")
    Bv = tr.triple(tr.sub(tr.sub(tr.mul(CB, xz, "b·xz"), xx), tr.triple(zz, "3zz")), "B")
    C = tr.triple(tr.sub(xx, zz), "C")
    lo, up = tr.sub(yy, A), tr.add(yy, A, "yy+A")
    x = tr.sub(tr.mul(xy, lo, "xy·lo"), tr.mul(yz, Bv, "yz·B"))
    y = tr.add(tr.mul(up, lo, "up·lo"), tr.mul(C, Bv, "C·B"), "Y3")
    z = tr.add(tr.mul(yz, up, "yz·up"), tr.mul(xy, C, "xy·C"), "Z3")
    return x, y, z


def _cross(tr, p1, p2, q1, q2, first, second, op):
    both = tr.mul(tr.add(p1, p2, "p: " + op), tr.add(q1, q2, "q: " + op), "(p)(q): " + op)
    return tr.sub(tr.sub(both, first), second)


def add_general(tr, p, q):
    """t256_add"""
    xx, yy, zz = tr.mul(p[0], q[0], "xx"), tr.mul(p[1], q[1], "yy"), tr.mul(p[2], q[2], "zz")
    xy = _cross(tr, p[0], p[1], q[0], q[1], xx, yy, "x+y")
    xz = _cross(tr, p[0], p[2], q[0], q[2], xx, zz, "x+z")
    yz = _cross(tr, p[1], p[2], q[1], q[2], yy, zz, "y+z")
    return _add_tail(tr, xx, yy, zz, xy, xz, yz)


def add_mixed(tr, p, q):
    """t256_add_mixed: q is a table entry (x, y)"""
    xx, yy = tr.mul(p[0], q[0], "xx"), tr.mul(p[1], q[1], "yy")
    xy = _cross(tr, p[0], p[1], q[0], q[1], xx, yy, "x+y")
    xz = tr.add(p[0], tr.mul(q[0], p[2], "q.x·p.z"), "xz")
    yz = tr.add(p[1], tr.mul(q[1], p[2], "q.y·p.z"), "yz")
    return _add_tail(tr, xx, yy, p[2], xy, xz, yz)


def lanes_log(n_gens):
    """log2 of the lanes a row of a SMALL call has: the least power of two >= n_gens + 1, at most 64"""
    log_w = 0
    while log_w < 6 and (1 << log_w) < n_gens + 1:
        log_w += 1
    return log_w


def walk_share(tr, entry, z, blind, t, log_w):
    """t256_walk_share of lane t: `entry(j, w, d)` is the table's d·2^(8w)·P_j as representations (x, y)"""
    W, n = 1 << log_w, len(z)
    log_per = 0 if log_w >= 5 else 5 - log_w
    acc = IDENTITY
    for i in range((n + 1) << log_per):
        j, r = i >> log_per, i & ((1 << log_per) - 1)
        w = ((t + W - (j & (W - 1))) & (W - 1)) + (r << log_w)
        if w >= 32:
            continue
        d = ((z[j] if j < n else blind) >> (8 * w)) & 255
        if d:
            tr.stage, tr.where = "mixed", (t, j, w)
            acc = add_mixed(tr, acc, entry(j, w, d))
    return acc


def inv(tr, a):
    """ft256_inv: to_mont(1), then square and multiply down the bits of p_T - 2; step 511 is the last, a product with a"""
    tr.stage, tr.where = "inv", None
    r = tr.mul(1, R2, "to_mont(1)")
    for s in range(512):
        tr.where = s
        if s % 2 == 0:
            r = tr.mul(r, r, "sqr")
        elif ((PT - 2) >> (255 - (s >> 1))) & 1:
            r = tr.mul(r, a, "last" if s == 511 else "mul")
    return r


@functools.lru_cache(maxsize=None)
def _entry_of(point, w, d):
    x, y = V.mul(d << (8 * w), point)
    return mont(x), mont(y)


def entries(points, h):
    """the tables of a set, an entry computed where a row asks for it"""
    pts = list(points) + [h]
    return lambda j, w, d: _entry_of(pts[j], w, d)


def full_tables(points, h):
    """the same with every entry made beforehand by additions, for many rows over one small set"""
    tabs = []
    for p in list(points) + [h]:
        tab, base = [], p
        for w in range(32):
            acc, row = None, []
            for d in range(255):
                acc = V.add(acc, base)
                row.append((mont(acc[0]), mont(acc[1])))
            tab.append(row)
            base = V.add(acc, base)
        tabs.append(tab)
    return lambda j, w, d: tabs[j][w][d - 1]


def trace_row(entry, z, blind, missed=False):
    """One row of a small call as the device runs it -> (the affine point or None, the Trace).  The finish's inversion runs
    on an identity too (zero gives zero); its two products and conversions do not."""
    tr = Trace(missed)
    log_w = lanes_log(len(z))
    acc = [walk_share(tr, entry, z, blind, t, log_w) for t in range(1 << log_w)]
    s = (1 << log_w) >> 1
    while s:
        for t in range(s):
            tr.stage, tr.where = "butterfly s=%d" % s, t
            acc[t] = add_general(tr, acc[t], acc[t + s])
        s >>= 1
    X, Y, Z = acc[0]
    zinv = inv(tr, Z)
    if Z == 0:
        return None, tr
    tr.stage, tr.where = "finish", None
    x = tr.mul(tr.mul(X, zinv, "x·zinv"), 1, "from_mont x")
    y = tr.mul(tr.mul(Y, zinv, "y·zinv"), 1, "from_mont y")
    return (x, y), tr


def sites(tr):
    return {(stage, op) for stage, op, _ in tr.hits}


# ---- the vectors -------------------------------------------------------------------------------------------------------------------
# a family is ONE generator set and its rows: the steered ones, each with the (stage, operation) the model must show for it, and
# two unsteered ones (site None)
Row = collections.namedtuple("Row", "name z blind site")
Family = collections.namedtuple("Family", "name gens rows")


def _search(rng, make):
    for _ in range(TRIES):
        got = make(rng)
        if got is not None:
            return got
    raise RuntimeError("search bound exhausted")


def _small(rng):
    return unmont(rng.randrange(1, 1 << 200))


def _hits(points, z, site):
    return site in sites(trace_row(entries(points, H), z, 0)[1])


def _lone(rng, n, j, make, site, scalar=1):
    """a generator for place j of an n-generator set from `make(rng)` (a point or None), accepted where the model shows that
    the row scalar·e_j hits `site`; the other places do not enter that row"""
    def attempt(g):
        pt = make(g)
        if pt is None:
            return None
        z = [0] * n
        z[j] = scalar
        return pt if _hits([pt if i == j else G for i in range(n)], z, site) else None
    return _search(rng, attempt)


def _one_hot(n, j, scalar=1):
    return tuple(scalar if i == j else 0 for i in range(n))


def _family(name, rng, points, steered):
    n = len(points)
    rows = list(steered) + [Row("unsteered %d" % i, tuple(rng.randrange(Q) for _ in range(n)), rng.randrange(Q), None) for i in range(2)]
    return Family(name, V.PointGens(points, H), tuple(rows))


def family_finish(which):
    """finish_x, finish_y: the affine x (y) of the row's sum has a representation below 2^200, so X·Z^-1 (Y·Z^-1) in
    t256_write_compressed holds rho + p_T; one generator for either parity of y"""
    rng = random.Random(0x7F1A0 + ord(which))
    site = ("finish", which + "·zinv")

    def make(odd):
        if which == "x":
            return lambda g: lift_x(_small(g), odd)

        def by_y(g):
            y = _small(g)
            x = x_of_y(y) if y & 1 == odd else None
            return None if x is None else (x, y)
        return by_y
    points = [_lone(rng, 2, j, make(odd), site) for j, odd in enumerate((1, 0))]
    return _family("finish_" + which, rng, points, [Row("finish_%s y %s" % (which, "odd" if j == 0 else "even"), _one_hot(2, j), 0, site) for j in range(2)])


def family_inv_last():
    """the sum of the row e_j is (x y^7 : y^8 : y^7): y^7 = 1 / (rho 2^-256), so the last product of ft256_inv, which makes
    Z^-1, holds rho + p_T"""
    rng = random.Random(0x7F1A3)
    site = ("inv", "last")

    def make(g):
        y = kth_root(pow(_small(g), -1, PT), 7)
        x = None if y is None else x_of_y(y)
        return None if x is None else (x, y)
    points = [_lone(rng, 2, j, make, site) for j in range(2)]
    return _family("inv_last", rng, points, [Row("inv_last lane %d" % j, _one_hot(2, j), 0, site) for j in range(2)])


MIXED_SUM_DELTAS = (0, 1 << 200, DELTA_MAX)             # the line of 2^100 misses the curve


def family_mixed_sum():
    """generators with mont(x) + mont(y) = p_T + delta: the `ft256_add(q.x, q.y)` of t256_add_mixed on the table entry that IS
    the generator.  mont(x + y) = delta fixes the line x + y = c, so there is no search beyond the cubic's roots: a delta whose
    line misses the curve raises."""
    rng = random.Random(0x7F1A4)
    site = ("mixed", "q: x+y")
    points = []
    for delta in MIXED_SUM_DELTAS:
        pt = on_line(unmont(delta))
        if pt is None or mont(pt[0]) + mont(pt[1]) != PT + delta:
            raise RuntimeError("no generator for delta = %x" % delta)
        points.append(pt)
    rows = [Row("mixed_sum delta=%x" % d, _one_hot(3, j), 0, site) for j, d in enumerate(MIXED_SUM_DELTAS)]
    return _family("mixed_sum", rng, points, rows)


BUTTERFLY_TRIED = ("zz at s=1", "yy at s=2")             # both reached; xx and the cross terms were not tried: they ask for a
                                                         # root of a polynomial of degree 11 in a coordinate of the generator


def family_butterfly():
    """Three generators.  Of the row ([1, 1, 0], 0) lanes 0 and 1 reach the last step as (x y^3 : y^4 : y^3), so its `zz` is
    (y_0 y_1)^3: y_1 = (rho 2^-256)^(1/3) / y_0.  Of the row ([1, 0, 1], 0) lanes 0 and 2 meet in the first step, s = 2, as
    (x y : y^2 : y), so its `yy` is (y_0 y_2)^2: y_2 = (rho 2^-256)^(1/2) / y_0."""
    rng = random.Random(0x7F1A5)
    p0 = _search(rng, lambda g: lift_x(g.randrange(PT), g.randrange(2)))
    inv_y0 = pow(p0[1], -1, PT)

    def partner(root, place, z, site):
        def attempt(g):
            r = root(_small(g))
            x = None if r is None else x_of_y(r * inv_y0 % PT)
            if x is None:
                return None
            pt = (x, r * inv_y0 % PT)
            pts = [p0, G, G]
            pts[place] = pt
            return pt if _hits(pts, z, site) else None
        return _search(rng, attempt)
    zz, yy = ("butterfly s=1", "zz"), ("butterfly s=2", "yy")
    p1 = partner(lambda v: kth_root(v, 3), 1, (1, 1, 0), zz)
    p2 = partner(sqrt_pt, 2, (1, 0, 1), yy)
    return _family("butterfly", rng, [p0, p1, p2], [Row("butterfly zz", (1, 1, 0), 0, zz), Row("butterfly yy", (1, 0, 1), 0, yy)])


TABLE_ENTRIES = ((5, 1), (0, 0x9C), (17, 200))           # (w, d): one w >= 1, one d >= 2, one both


def family_table_entry():
    """finish_x reached through a table entry other than row 0 entry 0: the generator is (d 2^(8w))^-1 T for a steered T,
    and the row ([d 2^(8w)], 0) sums to T"""
    rng = random.Random(0x7F1A6)
    site = ("finish", "x·zinv")
    n = len(TABLE_ENTRIES)
    points, rows = [], []
    for j, (w, d) in enumerate(TABLE_ENTRIES):
        k = d << (8 * w)
        make = lambda g, k=k: (lambda T: None if T is None else V.mul(pow(k, -1, Q), T))(lift_x(_small(g), g.randrange(2)))
        points.append(_lone(rng, n, j, make, site, scalar=k))
        rows.append(Row("table_entry w=%d d=%d" % (w, d), _one_hot(n, j, k), 0, site))
    return _family("table_entry", rng, points, rows)


FAMILIES = (("finish_x", lambda: family_finish("x")), ("finish_y", lambda: family_finish("y")), ("inv_last", family_inv_last),
            ("mixed_sum", family_mixed_sum), ("butterfly", family_butterfly), ("table_entry", family_table_entry))
COUNTS = {"finish_x": 2, "finish_y": 2, "inv_last": 2, "mixed_sum": 3, "butterfly": 2, "table_entry": 3}     # steered rows


@functools.lru_cache(maxsize=None)
def families():
    """family name -> Family, built once per process"""
    return {name: make() for name, make in FAMILIES}


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's (status, 33 bytes) of every row of the family"""
    fam = families()[name]
    return tuple(fam.gens.commit(list(r.z), r.blind) for r in fam.rows)
