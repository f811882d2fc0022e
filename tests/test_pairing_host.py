"""csrc/pairing.hpp on the HOST (g++ build of tests/cpp/test_pairing.cpp) against the oracle's restatement of ark-ec's
BN254 pairing (oracle/ark_files.py): the Fq12 tower, the Frobenius constants (frob_k(x) == x^(q^k)), cyclotomic squaring,
G2Prepared coefficients, the multi-Miller loop with identity skips, the final exponentiation byte for byte, the group
checks and prepare_inputs.  Pure CPU."""
import os
import subprocess
import sys

import pytest

import ark_files
import bn254_oracle as o
from conftest import ROOT
import verify_vectors as V

Q, R = o.Q, o.R


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pairing") / "test_pairing")
    src = os.path.join(ROOT, "tests", "cpp", "test_pairing.cpp")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(line):
        p.stdin.write(line + "\n")
        p.stdin.flush()
        out = p.stdout.readline().strip()
        assert out != "ERR", line[:40]
        return out
    yield ask
    p.stdin.close()
    p.wait(timeout=30)


def f12hex(f):
    return ark_files.fq12_bytes(f).hex()


def test_constants_script_matches_header():
    """the constants pairing.hpp carries are the ones tools/pairing_consts.py derives"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pairing_consts.py")], capture_output=True, text=True, check=True)
    hdr = open(os.path.join(ROOT, "crescent-credentials_amd", "csrc", "pairing.hpp")).read().replace(" ", "")
    for line in r.stdout.splitlines():
        name = line.split("uint32_t")[1].split("[")[0].strip()
        body = line.split("=", 1)[1].replace(" ", "").rstrip(";")
        if name in ("TWIST_MUL_BY_Q_X",):                  # = FROB6_C1_1, which the header uses for it
            continue
        if name == "TWO_INV":
            body = body[1:body.index("}") + 1]
        body = body.replace("0x00000000u", "0")
        assert name in hdr and body in hdr.replace("0x00000000u", "0"), name


def test_fq12_arithmetic(tool):
    rng = V.rng(1)
    for _ in range(3):
        a, b = V.random_f12(rng), V.random_f12(rng)
        assert tool("f12 mul %s %s" % (f12hex(a), f12hex(b))) == f12hex(o._f12_mul(a, b))
        assert tool("f12 sqr %s" % f12hex(a)) == f12hex(o._f12_mul(a, a))
        assert tool("f12 inv %s" % f12hex(a)) == f12hex(o._f12_inv(a))
        assert tool("f12 conj %s" % f12hex(a)) == f12hex(o._f12_pow(a, Q ** 6))
        for k in (1, 2, 3):
            assert tool("f12 frob%d %s" % (k, f12hex(a))) == f12hex(o._f12_pow(a, Q ** k)), k


def test_cyclotomic_square(tool):
    rng = V.rng(2)
    a = V.random_f12(rng)
    c = o._f12_pow(a, (Q ** 6 - 1) * (Q ** 2 + 1))          # in the cyclotomic subgroup
    assert tool("f12 cyc %s" % f12hex(c)) == f12hex(o._f12_mul(c, c))
    assert tool("f12 cyc %s" % f12hex(a)) != f12hex(o._f12_mul(a, a))     # and it is a different map off the subgroup


def _coeff_hex(pq):
    return b"".join(ark_files._fq2_bytes(c0) + ark_files._fq2_bytes(c1) + ark_files._fq2_bytes(c2)
                    for c0, c1, c2 in pq["ell_coeffs"]).hex()


def test_g2_prepare(tool):
    for k in (1, 0xDEADBEEF, R - 5):
        Qp = V.g2(k)
        pq = ark_files.g2_prepare(Qp)
        assert len(pq["ell_coeffs"]) == 91
        assert tool("prep %s" % V.g2_hex(Qp)) == _coeff_hex(pq), k


@pytest.mark.parametrize("nf", [0, 1, 3])
def test_multi_miller_loop(tool, nf):
    P = [V.g1(11), V.g1(12), V.g1(13)]
    Qs = [V.g2(21), V.g2(22), V.g2(23)]
    cases = [
        [(P[0], Qs[0]), (None, Qs[1]), (None, Qs[2])],                  # one pair
        [(P[0], Qs[0]), (P[1], Qs[1]), (None, None)],                   # two
        [(P[0], Qs[0]), (P[1], Qs[1]), (P[2], Qs[2])],                  # three
        [(P[0], None), (P[1], Qs[1]), (P[2], Qs[2])],                   # first skipped by its G2 point
        [(None, None), (None, None), (None, None)],                     # nothing: f = 1
    ]
    for pairs in cases:
        want = ark_files.multi_miller_loop([(p, ark_files.g2_prepare(q)) for p, q in pairs])
        line = "miller %d " % nf + " ".join("%s %s" % (V.g1_hex(p), V.g2_hex(q)) for p, q in pairs)
        assert tool(line) == f12hex(want), pairs


def test_final_exponentiation(tool):
    rng = V.rng(3)
    f = ark_files.multi_miller_loop([(V.g1(5), ark_files.g2_prepare(V.g2(7)))])
    for x in (f, V.random_f12(rng)):
        assert tool("fexp %s" % f12hex(x)) == f12hex(ark_files.final_exponentiation(x))
    assert tool("fexp %s" % f12hex([0] * 12)) == "NONE"
    # the pairing is bilinear through the whole chain: e(5 G1, 7 G2) == e(35 G1, G2)
    g = ark_files.multi_miller_loop([(V.g1(35), ark_files.g2_prepare(V.g2(1)))])
    assert tool("fexp %s" % f12hex(g)) == tool("fexp %s" % f12hex(f))


def test_group_checks(tool):
    rng = V.rng(4)
    assert tool("check %s g1" % V.g1_hex(V.g1(9))) == "1"
    assert tool("check %s g1" % V.g1_hex((1, 3))) == "0"
    B = V.g2(77)
    assert tool("check %s g2" % V.g2_hex(B)) == "1"
    assert tool("check %s sub" % V.g2_hex(B)) == "1"
    assert tool("check %s g2" % V.g2_hex((B[0], (B[1][0], (B[1][1] + 1) % Q)))) == "0"
    T = V.twist_point_outside_g2(rng)
    assert tool("check %s g2" % V.g2_hex(T)) == "1"
    assert tool("check %s sub" % V.g2_hex(T)) == "0"


def test_prepare_inputs(tool):
    rng = V.rng(5)
    vk = {"gamma_abc_g1": [V.g1(rng.randrange(R)) for _ in range(4)]}
    xs = [rng.randrange(R), 0, R - 1]
    want = o.G1.to_affine(o.prepare_inputs(vk, xs))
    line = "inputs 3 " + " ".join(V.g1_hex(p) for p in vk["gamma_abc_g1"]) + " " + \
        " ".join(int(x).to_bytes(32, "little").hex() for x in xs)
    assert tool(line) == V.g1_hex(want)


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_fixed_base_walk_and_254_step_chain(tool, group):
    """csrc/fixed_base.hpp's build_tables + fixed_base_mul and its scalar_mul_254_mixed against the oracle's k·P:
    the edges of a window (0, 1, 255, 256), the top byte empty, r - 1, every digit 0xFF (an unreduced scalar for the walk,
    2^254 - 1 for the chain, both >= r) and two seeded values"""
    rng = V.rng(6)
    curve, P, hx = (o.G1, V.g1(0xC0FFEE), V.g1_hex) if group == "g1" else (o.G2, V.g2(0xC0FFEE), V.g2_hex)
    common = [0, 1, 255, 256, 2 ** 248 - 1, R - 1, rng.randrange(R), rng.randrange(R)]
    for cmd, ks in (("fb", common + [2 ** 256 - 1]), ("mul254", common + [2 ** 254 - 1])):
        for k in ks:
            want = curve.to_affine(curve.mul_affine(P, k))
            assert tool("%s %s %s %s" % (cmd, group, hx(P), k.to_bytes(32, "little").hex())) == hx(want), (cmd, hex(k))
