"""csrc/ft256.hpp and csrc/t256.hpp on the HOST (g++ build of tests/cpp/test_t256.cpp, a program with its own main) against
Python integers and tests/t256_vectors.py: the field at p_T's edges and on seeded pairs, single operations STEERED to the
case "no ninth bit, yet not below p_T" of the reduction (2^256 - p_T is about 2^224, so random operands meet it once in
2^32), the inversion, the complete addition on equal, opposite and identity operands, the table walk on structured scalars,
the one writer of the compressed form on the identity and both parities, the table builder for three bases, the refusals
cg_t256_gens_load makes before any HIP call, and whole rows.  The same program, built with the address and
undefined-behaviour sanitizers, answers the same requests on its own.  Pure CPU.

The integer model of the rare case is tests/steer_vectors.py's, restated for this modulus (that file's tables hold P-256's two
primes only):
    mont(v) = v 2^256 mod p;  pre(a, b) = (a b + ((-a b p^-1) mod 2^256) p) >> 256 is what a word-by-word Montgomery product of
    the representations a and b holds before its conditional subtraction; a product hits the case iff p <= pre < 2^256, a sum
    of representations A and B iff p <= A + B < 2^256."""
import os
import random
import subprocess

import pytest

from conftest import ROOT
import t256_vectors as V

PT, Q, G = V.PT, V.Q, V.G
R = 1 << 256
SRC = os.path.join(ROOT, "tests", "cpp", "test_t256.cpp")
EDGES = [0, 1, 2, PT - 1, PT - 2, 1 << 255, (1 << 255) + 1, (1 << 255) - 1, 1 << 224]
ZERO_WINDOWS = (0xAB << 240) | (0x0F << 120) | 0x10      # most windows are zero
SCALARS = [0, 1, 2, 255, 256, Q - 1, Q - 2, V.TOP_DIGIT, ZERO_WINDOWS, int("01" * 32, 16)]
be = lambda v: int(v).to_bytes(32, "big").hex()
le = lambda v: V.scalar_bytes(v).hex()
pt = lambda p: V.uncompressed(p).hex()

_PINV, _RINV = pow(PT, -1, R), pow(R, -1, PT)
mont = lambda v: v * R % PT
unmont = lambda rep: rep * _RINV % PT


def pre(a, b):
    t = a * b
    return (t + (-t * _PINV) % R * PT) >> 256


rare = lambda value: PT <= value < R
mul_hits = lambda a, b: rare(pre(mont(a), mont(b)))            # a, b: values
add_hits = lambda a, b: rare(mont(a) + mont(b))
from_words_hits = lambda x: rare(pre(x, R * R % PT))


def ask_all(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = r.stdout.split()
    assert len(out) == len(lines) and "ERR" not in out, r.stdout[-2000:]
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("t256") / "test_t256")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", path, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def compare(exe, lines, want):
    got = ask_all(exe, lines)
    for line, g, w in zip(lines, got, want):
        assert g == w, line[:160]


# ---- the field -------------------------------------------------------------------------------------------------------------------
def field_lines(n_random, n_inv):
    rng = random.Random(0xF7256)
    pairs = [(a, b) for a in EDGES for b in EDGES] + [(rng.randrange(PT), rng.randrange(PT)) for _ in range(n_random)]
    lines, want = [], []
    for a, b in pairs:
        lines += ["fadd %s %s" % (be(a), be(b)), "fsub %s %s" % (be(a), be(b)), "fmul %s %s" % (be(a), be(b))]
        want += [be((a + b) % PT), be((a - b) % PT), be(a * b % PT)]
    for a in EDGES + [rng.randrange(1, PT) for _ in range(n_inv)]:
        lines += ["finv " + be(a), "fneg " + be(a), "fsqr " + be(a)]
        want += [be(pow(a, -1, PT) if a else 0), be(-a % PT), be(a * a % PT)]
    for v, ok in ((0, 1), (PT - 1, 1), (PT, 0), (PT + 1, 0), (R - 1, 0), (1 << 255, 1), (PT - (1 << 128), 1), (PT + (1 << 128), 0)):
        lines.append("fbelow " + be(v))
        want.append(str(ok))
    lines.append("fconsts")
    want.append("1")
    return lines, want


def test_field_at_the_edges_on_seeded_pairs_and_the_inversion(exe):
    lines, want = field_lines(10000, 48)
    compare(exe, lines, want)
    assert 2 * (PT - 1) >= R                                                   # the sum Fp<P> cannot hold
    assert (-pow(PT, -1, 1 << 32)) % (1 << 32) == 0x0f646959


def _search(rng, make, tries=4000):
    for _ in range(tries):
        got = make(rng)
        if got is not None:
            return got
    raise RuntimeError("search bound exhausted")


def steered_lines():
    """single operations whose sum or Montgomery product lands in the rare case, each shown by the model to land there"""
    rng = random.Random(0x57EE7)
    lines, want = [], []

    def product(g):
        # a product whose result has a small representation rho is rho or rho + p before the subtraction
        b = g.randrange(1, PT)
        a = unmont(g.randrange(1, 1 << 200)) * pow(b, -1, PT) % PT
        return (a, b) if mul_hits(a, b) else None

    def square(g):
        v = unmont(g.randrange(1, 1 << 200))
        a = pow(v, (PT + 1) // 4, PT)                                          # p_T = 3 mod 4
        return a if a * a % PT == v and mul_hits(a, a) else None

    def word_entry(g):
        x = unmont(g.randrange(1, 1 << 200))
        return x if from_words_hits(x) else None

    for _ in range(6):
        a, b = _search(rng, product)
        lines.append("fmul %s %s" % (be(a), be(b)))
        want.append(be(a * b % PT))
    for _ in range(4):
        a = _search(rng, square)
        lines += ["fsqr " + be(a), "fmul %s %s" % (be(a), be(a))]
        want += [be(a * a % PT)] * 2
    for _ in range(4):
        x = _search(rng, word_entry)                                           # ft256_from_words itself takes the branch
        lines += ["fadd %s %s" % (be(x), be(0)), "fmul %s %s" % (be(x), be(1)), "finv " + be(x)]
        want += [be(x), be(x), be(pow(x, -1, PT))]
    # sums of representations in [p, 2^256): the representations add up to p + delta
    for delta in (0, 1, 1 << 100, R - 1 - PT):
        A = rng.randrange(delta + 1, PT)
        a, b = unmont(A), unmont(PT + delta - A)
        assert add_hits(a, b)
        lines.append("fadd %s %s" % (be(a), be(b)))
        want.append(be((a + b) % PT))
    return lines, want


def test_single_operations_steered_to_the_rare_case_of_the_reduction(exe):
    lines, want = steered_lines()
    assert len(lines) == 6 + 8 + 12 + 4
    compare(exe, lines, want)
    # random operands do not get there: none of 2000 seeded products does
    rng = random.Random(1)
    assert not any(mul_hits(rng.randrange(PT), rng.randrange(PT)) for _ in range(2000))


# ---- the group -----------------------------------------------------------------------------------------------------------------
def group_lines(n_random):
    rng = random.Random(0x67256)
    A, B = V.mul(rng.randrange(Q), G), V.mul(rng.randrange(Q), G)
    lines, want = [], []
    for p, q in ((A, A), (A, V.neg(A)), (A, None), (None, A), (None, None), (A, B), (G, G), (G, V.neg(G))):
        lines.append("gadd %s %s" % (pt(p), pt(q)))
        want.append(pt(V.add(p, q)))
    for p, q in ((A, A), (A, V.neg(A)), (None, A), (A, B)):
        lines.append("gmixed %s %s" % (pt(p), pt(q)))
        want.append(pt(V.add(p, q)))
    for p in (A, G, None):
        lines.append("gdbl " + pt(p))
        want.append(pt(V.add(p, p)))
    for p, code in ((G, 0), (A, 0), ((G[0], G[1] + 1), 2), ((PT, G[1]), 1), ((R - 1, G[1]), 1), ((G[0], PT), 1), ((0, 1), 2), (None, 3)):
        lines.append("read " + (be(p[0]) + be(p[1]) if p else pt(None)))
        want.append(str(code))
    for k in SCALARS + [rng.randrange(Q) for _ in range(n_random)]:
        for base in (G, A):
            lines.append("walk %s %s" % (pt(base), le(k)))
            want.append(pt(V.mul(k, base)))
    odd, even = [next(p for p in (V.mul(k, G) for k in range(1, 50)) if p[1] & 1 == bit) for bit in (1, 0)]
    for p in (None, odd, even, A):
        lines.append("compress " + pt(p))
        want.append(V.compressed(p).hex())
    assert want[-4] == "40" + "00" * 32 and want[-3][:2] == "80" and want[-2][:2] == "00"
    return lines, want


def test_complete_addition_on_every_case_the_walk_and_the_compressed_writer(exe):
    lines, want = group_lines(24)
    assert sum(w == pt(None) for w in want) >= 5                               # P + (-P), O + O, 2 O and 0 P among them
    compare(exe, lines, want)


def test_tables_of_three_bases(exe):
    rng = random.Random(0x7AB)
    for base in (G, V.mul(rng.randrange(Q), G), V.neg(G)):
        first, middle, last = ask_all(exe, ["tabrow %s 0" % pt(base), "tabrow %s 17" % pt(base), "tabrow %s 31" % pt(base)])
        for row, start in ((first, base), (middle, V.mul(1 << 136, base)), (last, V.mul(1 << 248, base))):
            assert len(row) == 255 * 128
            acc = None
            for d in range(255):
                acc = V.add(acc, start)
                assert row[128 * d:128 * d + 128] == pt(acc), d


def refusal_lines():
    gens = V.make_gens(0x6E5, 3)
    g, h = gens.g_xy, gens.h_xy
    off = be(gens.points[1][0]) + be((gens.points[1][1] + 1) % PT)
    big = be(PT) + be(gens.points[1][1])
    swap = lambda j, new: (g[:64 * j] + bytes.fromhex(new) + g[64 * j + 64:]).hex()
    cases = [(g.hex(), h.hex(), "0:0"), (swap(1, off), h.hex(), "2:1"), (swap(2, big), h.hex(), "1:2"), (swap(0, "00" * 64), h.hex(), "3:0"),
             (g.hex(), off, "2:3"), (g.hex(), big, "1:3"), (g.hex(), "00" * 64, "3:3"), (swap(2, be(5) + be(R - 1)), h.hex(), "1:2")]
    return ["gens 3 %s %s" % (a, b) for a, b, _ in cases], [w for _, _, w in cases]


def test_refusals_of_the_generator_loader(exe):
    compare(exe, *refusal_lines())


def row_lines(n_random):
    rng = random.Random(0x60E)
    gens = V.make_gens(0x6E6, 3)
    rows = [([0, 0, 0], 0), ([1, Q - 1, V.TOP_DIGIT], 1), ([Q, 1, 1], 5), ([1, 1, R - 1], 5), ([1, 1, 1], Q), ([0, 1, 0], 0)]
    rows += [(V.mixed_scalars(rng, 3), rng.randrange(Q)) for _ in range(n_random)]
    lines, want = [], []
    for z, blind in rows:
        st, out = gens.commit(z, blind)
        if st == V.MADE:
            assert out == gens.commit_term_by_term(z, blind)
        lines.append("row 3 %s %s %s %s" % (gens.g_xy.hex(), gens.h_xy.hex(), "".join(le(v) for v in z), le(blind)))
        want.append("%d%s" % (st, out.hex()))
    assert want[0] == "1" + V.IDENTITY_COMPRESSED.hex() and [w[0] for w in want[2:5]] == ["2"] * 3
    V.assert_both_parities([bytes.fromhex(w[1:]) for w in want])
    return lines, want


def test_whole_rows_with_both_statuses(exe):
    compare(exe, *row_lines(10))


def test_sanitized_build_answers_the_same(tmp_path):
    path = str(tmp_path / "test_t256_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", path, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines, want = field_lines(300, 6)
    for a, b in (steered_lines(), group_lines(2), refusal_lines(), row_lines(3)):
        lines, want = lines + list(a), want + list(b)
    assert ask_all(path, lines + ["tabrow %s 31" % pt(G)])[:-1] == want
