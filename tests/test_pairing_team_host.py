"""csrc/pairing_team.hpp on the HOST (g++ build of tests/cpp/test_pairing_team.cpp): the team pairing of the verifiers'
latency arrangement against the oracle's restatement of ark-ec (oracle/ark_files.py) and, inside the program, against
pairing.hpp's serial functions - byte for byte.  The program runs one lane over a shared array that counts phases and
aborts on a read or write that a missing sync() would turn into a race on the device, so every value below is also a
statement that the phases are ordered.  Pure CPU."""
import os
import subprocess

import pytest

import ark_files
import bn254_oracle as o
from conftest import ROOT
import verify_vectors as V

Q = o.Q
SRC = os.path.join(ROOT, "tests", "cpp", "test_pairing_team.cpp")


def _build(exe, *flags):
    r = subprocess.run(["g++", "-std=c++17", *flags, "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("pairing_team") / "test_pairing_team"), "-O2")


@pytest.fixture(scope="module")
def tool(exe):
    p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(line):
        p.stdin.write(line + "\n")
        p.stdin.flush()
        out = p.stdout.readline().strip()
        assert out not in ("ERR", "MISMATCH", ""), (out, line[:40])
        return out
    yield ask
    p.stdin.close()
    assert p.wait(timeout=30) == 0


def f12hex(f):
    return ark_files.fq12_bytes(f).hex()


P = [V.g1(11), V.g1(12), V.g1(13)]
QS = [V.g2(21), V.g2(22), V.g2(23)]


def _miller_line(nf, mask, pairs):
    return "miller %d %d " % (nf, mask) + " ".join("%s %s" % (V.g1_hex(p), V.g2_hex(q)) for p, q in pairs)


@pytest.fixture(scope="module")
def miller_want():
    """the oracle's Miller value of every subset of the three pairs, computed once"""
    prep = [ark_files.g2_prepare(q) for q in QS]
    return {mask: ark_files.multi_miller_loop([(P[j], prep[j]) if (mask >> j) & 1 else (None, ark_files.g2_prepare(None)) for j in range(3)])
            for mask in range(8)}


@pytest.mark.parametrize("nf", [0, 1, 3])
def test_team_multi_miller_loop_every_live_pattern(tool, miller_want, nf):
    """all eight live patterns of three random pairs, by the flag; all three false gives one"""
    pairs = list(zip(P, QS))
    for mask in range(8):
        assert tool(_miller_line(nf, mask, pairs)) == f12hex(miller_want[mask]), mask
    assert tool(_miller_line(nf, 0, pairs)) == f12hex([1] + [0] * 11)


@pytest.mark.parametrize("nf", [0, 1, 3])
def test_team_multi_miller_loop_identity_points(tool, miller_want, nf):
    """a pair dropped because one of its points is the identity, as the kernels derive `live`"""
    assert tool(_miller_line(nf, 7, [(P[0], None), (P[1], QS[1]), (P[2], QS[2])])) == f12hex(miller_want[6])
    assert tool(_miller_line(nf, 7, [(P[0], QS[0]), (None, QS[1]), (P[2], QS[2])])) == f12hex(miller_want[5])
    assert tool(_miller_line(nf, 7, [(None, None), (None, None), (None, None)])) == f12hex(miller_want[0])


def test_team_final_exponentiation(tool):
    rng = V.rng(3)
    f = ark_files.multi_miller_loop([(V.g1(5), ark_files.g2_prepare(V.g2(7)))])
    for x in (f, V.random_f12(rng)):
        assert tool("fexp %s" % f12hex(x)) == f12hex(ark_files.final_exponentiation(x))
    assert tool("fexp %s" % f12hex([0] * 12)) == "NONE"
    g = ark_files.multi_miller_loop([(V.g1(35), ark_files.g2_prepare(V.g2(1)))])
    assert tool("fexp %s" % f12hex(g)) == tool("fexp %s" % f12hex(f))            # e(5 G1, 7 G2) == e(35 G1, G2)


def test_team_fq12_operations(tool):
    rng = V.rng(1)
    a, b = V.random_f12(rng), V.random_f12(rng)
    assert tool("f12 mul %s %s" % (f12hex(a), f12hex(b))) == f12hex(o._f12_mul(a, b))
    assert tool("f12 inv %s" % f12hex(a)) == f12hex(o._f12_inv(a))
    assert tool("f12 conj %s" % f12hex(a)) == f12hex(o._f12_pow(a, Q ** 6))
    for k in (1, 2, 3):
        assert tool("f12 frob%d %s" % (k, f12hex(a))) == f12hex(o._f12_pow(a, Q ** k)), k
    c = o._f12_pow(a, (Q ** 6 - 1) * (Q ** 2 + 1))          # in the cyclotomic subgroup
    assert tool("f12 cyc %s" % f12hex(c)) == f12hex(o._f12_mul(c, c))


def test_team_comparisons(tool):
    rng = V.rng(7)
    a = V.random_f12(rng)
    one = [1] + [0] * 11
    assert tool("eq %s %s" % (f12hex(a), f12hex(a))) == "1"
    assert tool("isone %s" % f12hex(one)) == "1"
    assert tool("isone %s" % f12hex(a)) == "0"
    for i in range(12):                                     # a difference in any one coordinate
        b = list(a)
        b[i] = (b[i] + 1) % Q
        assert tool("eq %s %s" % (f12hex(a), f12hex(b))) == "0", i
        w = list(one)
        w[i] = (w[i] + 1) % Q
        assert tool("isone %s" % f12hex(w)) == "0", i


def test_race_check_trips_on_a_missing_sync(exe):
    """the toy sequence reads a product in the phase that writes it: the checked array must kill the program"""
    r = subprocess.run([exe, "toy"], capture_output=True, text=True)
    assert r.returncode != 0 and "race: read after another job's write" in r.stderr, (r.returncode, r.stdout, r.stderr)


def test_under_address_and_undefined_sanitizers(tmp_path):
    """the same stand-alone program built with -fsanitize=address,undefined, run once over every kind of command"""
    exe = _build(str(tmp_path / "test_pairing_team_san"), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    rng = V.rng(9)
    a = V.random_f12(rng)
    pairs = list(zip(P, QS))
    lines = [_miller_line(1, 7, pairs), _miller_line(0, 6, pairs), _miller_line(3, 5, pairs), _miller_line(1, 0, pairs),
             "fexp %s" % f12hex(a), "fexp %s" % f12hex([0] * 12), "f12 inv %s" % f12hex(a), "eq %s %s" % (f12hex(a), f12hex(a)),
             "isone %s" % f12hex(a)]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    out = r.stdout.split()
    assert len(out) == len(lines) and "MISMATCH" not in out and "ERR" not in out, out
    assert out[5] == "NONE" and out[7] == "1" and out[8] == "0"
