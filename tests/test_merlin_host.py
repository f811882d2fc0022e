"""csrc/merlin.hpp on the HOST (g++ build of tests/cpp/test_merlin.cpp) against the pure-Python Merlin of
tests/merlin_vectors.py, byte for byte: the known answers, every alignment of a message against the 166-byte rate, long
challenges, random sequences of calls, the two fixed transcript shapes the kernels use and the point compression in front
of them.  The same program, built with the address and undefined-behaviour sanitizers, runs the known answers on its own.
Pure CPU."""
import os
import random
import subprocess

import pytest

from conftest import ROOT
import merlin_vectors as MV

SRC = os.path.join(ROOT, "tests", "cpp", "test_merlin.cpp")


def hx(b):
    return bytes(b).hex() or "-"


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merlin") / "test_merlin")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(*words):
        p.stdin.write(" ".join(words) + "\n")
        p.stdin.flush()
        out = p.stdout.readline().strip()
        assert out != "ERR", words[0]
        return out
    ask.exe = exe
    yield ask
    p.stdin.close()
    p.wait(timeout=30)


def run_seq(tool, label, calls):
    """calls: ('a', label, msg) or ('c', label, n); returns (the tool's challenges, Python's), both hex"""
    t = MV.Transcript(label)
    words, want = ["seq", hx(label)], b""
    for kind, lab, x in calls:
        if kind == "a":
            t.append_message(lab, x)
            words += ["a", hx(lab), hx(x)]
        else:
            want += t.challenge_bytes(lab, x)
            words += ["c", hx(lab), str(x)]
    return tool(*words), want.hex()


def test_the_oracle_checks_itself():
    MV.self_check()


def test_known_answers(tool):
    got, want = run_seq(tool, b"test protocol", [("a", b"some label", b"some data"), ("c", b"challenge", 32)])
    assert got == want == MV.KAT0
    f, g, q = MV.KAT_RANGE_IN
    assert tool("range", hx(f), hx(g), hx(q)) == MV.KAT_RANGE_C + "00" + MV.KAT_RANGE_RHO + "00"
    for context, shape, want in MV.KAT_DLOG:
        st = MV.kat_statements(shape)
        bases = b"".join(b for s in st for b in s[0])
        got = tool("dlog", hx(context or b""), ",".join(map(str, shape)), hx(bases), hx(b"".join(s[1] for s in st)), hx(b"".join(s[2] for s in st)))
        assert got == want + "00", shape
    r = subprocess.run([tool.exe, "kat"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout


def test_every_message_length_against_the_rate(tool):
    """0..400 bytes in one append_message: each alignment of the boundary at 166, the next operation's two header bytes
    straddling it included"""
    rng = random.Random(1)
    for n in range(401):
        msg = bytes(rng.randrange(256) for _ in range(n))
        got, want = run_seq(tool, b"\0", [("a", b"m", msg), ("c", b"\0", 31), ("a", b"again", msg[:7]), ("c", b"\0", 31)])
        assert got == want, n


def test_long_challenges(tool):
    for n in (166, 167, 165, 332, 333):
        got, want = run_seq(tool, b"\0", [("a", b"x", b"y" * 40), ("c", b"long", n), ("c", b"next", 5)])
        assert got == want, n


def test_random_sequences(tool):
    rng = random.Random(2)
    for case in range(200):
        calls = []
        for _ in range(rng.randrange(1, 12)):
            lab = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 20)))
            if rng.random() < 0.6:
                calls.append(("a", lab, bytes(rng.randrange(256) for _ in range(rng.choice([0, 1, 8, 32, 64, 163, 166, 200, 340])))))
            else:
                calls.append(("c", lab, rng.choice([1, 31, 32, 64, 166, 170])))
        calls.append(("c", b"\0", 31))
        got, want = run_seq(tool, bytes(rng.randrange(256) for _ in range(rng.randrange(0, 30))), calls)
        assert got == want, case


def test_fixed_shapes(tool):
    """the two shapes as the kernels run them, on random bytes"""
    rng = random.Random(3)
    pt = lambda: bytes(rng.randrange(256) for _ in range(32))
    for _ in range(20):
        f, g, q = pt(), pt(), pt()
        c, rho = MV.range_challenges(f, g, q)
        assert tool("range", hx(f), hx(g), hx(q)) == (c + b"\0" + rho + b"\0").hex()
        slot, cfb, k, ped = [pt(), pt()], [pt() for _ in range(4)], [pt(), pt()], pt()
        want = MV.range_dleq_challenge(slot, cfb, k[0], k[1], ped, f)
        assert tool("dleq", hx(b"".join(slot)), hx(b"".join(cfb)), hx(b"".join(k)), hx(ped), hx(f)) == (want + b"\0").hex()


def test_compression(tool):
    """ml_compress_g1 against the compressed form the tests' own codec writes: points, their negatives and O"""
    import range_vectors as RV
    o = RV.o
    rng = random.Random(4)
    for _ in range(8):
        k = rng.randrange(1, RV.R)
        for P in (RV.g1(k), RV.g1(-k)):
            assert tool("compress", o.g1_uncompressed(P).hex()) == o.g1_compressed(P).hex()
    assert tool("compress", o.g1_uncompressed(None).hex()) == o.g1_compressed(None).hex()
    # arithmetic only: coordinates that no deserialisation accepts still give 32 bytes
    assert len(tool("compress", "ff" * 31 + "3f" + "ff" * 31 + "3f")) == 64


def test_sanitized_build_runs_the_known_answers(tmp_path):
    exe = str(tmp_path / "test_merlin_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "kat"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.stdout + r.stderr)[-3000:]
