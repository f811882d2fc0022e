"""tests/t256_vectors.py against itself: the curve's facts, the group law on the cases a test leans on, the two byte writers,
and the closed form every wide test uses - a row computed term by term equals (sum z_j k_j + blind k_h mod q)·G.  Pure Python;
it also fails on a tree without csrc/t256.hpp, whose constants it compares with the oracle's."""
import os
import random
import re

from conftest import ROOT
import t256_vectors as V

PT, Q, G = V.PT, V.Q, V.G


def test_curve_facts():
    assert V.A == PT - 3 and PT % 4 == 3 and PT > 1 << 255
    assert V.on_curve(G) and V.mul(Q, G) is None and V.mul(Q + 1, G) == G
    assert V.add(V.mul(Q - 1, G), G) is None
    # the order passes Fermat's test on fixed bases: enough for a constant that is P-256's well-known prime
    assert all(pow(a, Q - 1, Q) == 1 for a in (2, 3, 5, 7, 11))


def test_headers_state_the_oracles_constants():
    csrc = os.path.join(ROOT, "crescent-credentials_amd", "csrc")
    words = lambda v: [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]

    def array(text, name):
        body = re.search(r"constexpr uint32_t %s\[8\] = \{([^}]*)\}" % name, text).group(1)
        return [int(w.strip().rstrip("u"), 16) for w in body.split(",")]
    ft, t = open(os.path.join(csrc, "ft256.hpp")).read(), open(os.path.join(csrc, "t256.hpp")).read()
    assert array(ft, "p") == words(PT)
    assert array(ft, "r2") == words(pow(2, 512, PT))
    assert array(t, "b") == words(V.B)
    assert array(t, "y") == words(G[1])
    assert "return i == 0 ? 5u : 0u;" in t


def test_group_law_on_the_cases_the_tests_lean_on():
    rng = random.Random(0x7256)
    a, b, c = (V.mul(rng.randrange(1, Q), G) for _ in range(3))
    assert V.add(a, V.neg(a)) is None and V.add(a, None) == a and V.add(None, None) is None
    assert V.add(V.add(a, b), c) == V.add(a, V.add(b, c))
    assert V.add(a, a) == V.mul(2, a) and V.on_curve(V.add(a, b))
    k, m = rng.randrange(Q), rng.randrange(Q)
    assert V.mul(k, V.mul(m, G)) == V.mul(k * m, G)
    assert V.mul(V.TOP_DIGIT, G) == V.mul(0xFF, V.mul(1 << 248, G))


def test_byte_writers():
    assert V.compressed(None) == b"\x40" + bytes(32) and V.uncompressed(None) == bytes(64)
    p = V.mul(3, G)
    for pt in (p, V.neg(p)):
        c = V.compressed(pt)
        assert len(c) == 33 and c[0] == (0x80 if pt[1] & 1 else 0) and c[1:] == pt[0].to_bytes(32, "big")
        assert V.uncompressed(pt) == pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")
    assert p[1] & 1 != V.neg(p)[1] & 1                                          # p_T is odd: a point and its negative differ in parity
    V.assert_both_parities([V.compressed(p), V.compressed(V.neg(p))])
    assert V.scalar_bytes(1) == b"\x01" + bytes(31)
    assert V.factored_lens(3) == (2, 4) and V.factored_lens(13) == (64, 128) and V.factored_lens(2) == (2, 2)


def test_a_row_term_by_term_equals_the_closed_form():
    rng = random.Random(0xC105ED)
    for n in (1, 4, 9):
        gens = V.make_gens(rng.randrange(1 << 30), n)
        rows = [([rng.randrange(Q) for _ in range(n)], rng.randrange(Q)), (V.mixed_scalars(rng, n), rng.randrange(Q)), ([0] * n, 0),
                ([Q - 1] * n, Q - 1)]
        for z, blind in rows:
            st, out = gens.commit(z, blind)
            assert st == V.MADE and out == gens.commit_term_by_term(z, blind)
        assert gens.commit([0] * n, 0) == (V.MADE, V.IDENTITY_COMPRESSED)
        assert gens.commit([Q] + [0] * (n - 1), 0) == (V.MALFORMED, V.ZERO_ROW)
        assert gens.commit([0] * n, (1 << 256) - 1) == (V.MALFORMED, V.ZERO_ROW)
    # a blind that cancels the vector part: blind = -(sum z k) / k_h
    gens = V.make_gens(5, 3)
    z = [rng.randrange(Q) for _ in range(3)]
    blind = -gens.row_scalar(z, 0) * pow(gens.kh, -1, Q) % Q
    assert gens.commit(z, blind) == (V.MADE, V.IDENTITY_COMPRESSED) == (V.MADE, gens.commit_term_by_term(z, blind))


def test_hyrax_is_the_rows_of_the_matrix():
    rng = random.Random(0x4A8)
    gens = V.make_gens(77, 4)
    vars_ = [rng.randrange(Q) for _ in range(8)]
    blinds = [rng.randrange(Q) for _ in range(2)]
    st, out = V.hyrax(gens, 3, vars_, blinds)
    assert st == V.MADE and out == gens.commit(vars_[:4], blinds[0])[1] + gens.commit(vars_[4:], blinds[1])[1]
    vars_[6] = Q
    assert V.hyrax(gens, 3, vars_, blinds) == (V.MALFORMED, V.ZERO_ROW * 2)
