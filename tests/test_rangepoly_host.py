"""csrc/rangepoly.hpp on the HOST (g++ build of tests/cpp/test_rangepoly.cpp, one lane) against the Python restatement of
the polynomial stage of `RangeProof::prove_n_bits` (tests/range_vectors.py): every term scalar of every point of the three
calls - g~, q, the three witness quotients and the three blinded quotients - the three evaluations and the three
random_v, and the inputs each call reports as malformed.  Pure CPU."""
import itertools
import os
import random
import subprocess

import pytest

from conftest import ROOT
import range_vectors as RV

R = RV.R


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rangepoly") / "test_rangepoly")
    src = os.path.join(ROOT, "tests", "cpp", "test_rangepoly.cpp")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(cmd, n, m, r_, rand, c=None, rho=None):
        line = "%s %d %s %s" % (cmd, n.bit_length() - 1, RV.fes([m, r_]).hex(), RV.fes(rand).hex())
        for x in (c, rho):
            if x is not None:
                line += " " + RV.fe(x).hex()
        p.stdin.write(line + "\n")
        p.stdin.flush()
        out = p.stdout.readline().strip()
        assert out != "ERR", line[:60]
        return out
    yield ask
    p.stdin.close()
    p.wait(timeout=30)


def want_commit(n, m, rand):
    P = RV.polys(n, m, rand)
    return RV.fes([m] + rand[RV.F] + P.g + rand[RV.G] + [rand[RV.TM], rand[RV.TR]] + rand[RV.TF] + [rand[RV.TM]]).hex()


def want_quotient(n, m, rand, c):
    P = RV.polys(n, m, rand, c)
    assert P.rem[0] == 0 and P.rem[1] == 0 and not any(P.rem[2])           # the three divisions are exact
    return RV.fes(P.q + rand[RV.Q]).hex()


def want_open(n, m, rand, c, rho):
    P = RV.polys(n, m, rand, c, rho)
    terms = [x for wit, bl in zip(P.wit, P.blind) for x in wit + bl]
    assert len(terms) == 4 * n + 15
    return RV.fes(terms + P.evals + P.vs).hex()


@pytest.mark.parametrize("n", [2, 4, 32])
def test_every_vector_and_evaluation(tool, n):
    rng = random.Random(n)
    ms = [0, 1, 1 << (n - 1), (1 << n) - 1, rng.randrange(1 << n)]
    blindings = [(0, 0, 0), (0, 0, 1), tuple(rng.randrange(R) for _ in range(3))]
    cs = [0, 1, rng.randrange(R)]
    rhos = [rng.randrange(R), 2]
    for m, b, c, rho in itertools.product(ms, blindings, cs, rhos):
        rand = list(b) + [rng.randrange(R) for _ in range(15)]
        r_ = rng.randrange(R)
        what = (n, m, b, c, rho)
        assert tool("commit", n, m, r_, rand) == want_commit(n, m, rand), what
        assert tool("quotient", n, m, r_, rand, c) == want_quotient(n, m, rand, c), what
        assert tool("open", n, m, r_, rand, c, rho) == want_open(n, m, rand, c, rho), what


def test_degrees(tool):
    """deg q = deg w^ = 2n + 3 with a non-zero blinding; with none g~ stops at n - 1 and q at 2n - 3"""
    rng = random.Random(9)
    for n in (4, 32):
        rand = [rng.randrange(1, R) for _ in range(18)]
        P = RV.polys(n, 5 % (1 << n), rand, 7, 11)
        assert P.q[-1] and P.w_hat[-1] and P.g[-1]
        rand[:3] = [0, 0, 0]
        P = RV.polys(n, 5 % (1 << n), rand, 7, 11)
        assert P.g[n:] == [0, 0, 0] and not any(P.q[2 * n - 2:]) and P.q[2 * n - 3]


def test_rand_w_hat_that_cancels_gives_v_zero_and_no_hiding_term(tool):
    n, rho = 4, 12345
    rng = random.Random(10)
    rand = [rng.randrange(1, R) for _ in range(18)]
    # f_coeff rand_f + q_coeff rand_q = 0 with q_coeff = f_coeff (rho - 1): rand_f = -(rho - 1) rand_q
    rand[RV.F] = [(-(rho - 1) * x) % R for x in rand[RV.Q]]
    P = RV.polys(n, 9, rand, 3, rho)
    assert P.rand_w == [0, 0, 0] and P.vs[2] == 0 and P.blind[2] == [0, 0] and P.vs[0] and P.vs[1]
    assert tool("open", n, 9, 1, rand, 3, rho) == want_open(n, 9, rand, 3, rho)


def test_malformed_inputs(tool):
    n = 4
    rng = random.Random(11)
    good = [rng.randrange(1, R) for _ in range(18)]
    w = RV.o.root_of_unity(n)
    ask = lambda m=9, r_=1, rand=good, c=3, rho=5: [tool("commit", n, m, r_, rand), tool("quotient", n, m, r_, rand, c),
                                                   tool("open", n, m, r_, rand, c, rho)]
    bad = ["MALFORMED"] * 3
    assert "MALFORMED" not in ask()
    assert ask(m=1 << n) == bad and ask(m=R) == bad and ask(r_=R) == bad
    assert ask(m=(1 << n) - 1) != bad and "MALFORMED" not in ask(m=(1 << n) - 1)
    for i in range(18):
        assert ask(rand=good[:i] + [R] + good[i + 1:]) == bad, i
    for sl in (RV.F, RV.G, RV.Q):
        rand = list(good)
        rand[sl] = [0] * len(rand[sl])
        assert ask(rand=rand) == bad
        rand[sl.start] = 1
        assert "MALFORMED" not in ask(rand=rand)
    assert [x == "MALFORMED" for x in ask(c=R)] == [False, True, True]
    for rho in (R, 1, w, pow(w, 3, R)):                       # rho^n = 1, rho = 1 among them
        assert [x == "MALFORMED" for x in ask(rho=rho)] == [False, False, True], rho
    for m in (0, 1 << 32):                                    # n = 32: every 32-bit m, nothing above
        got = tool("commit", 32, m, 1, good)
        assert (got == "MALFORMED") == (m > 0)
