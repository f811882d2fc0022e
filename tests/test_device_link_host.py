"""csrc/sha256.hpp and csrc/device_link.hpp on the HOST (g++ build of tests/cpp/test_device_link.cpp): SHA-256 against hashlib
at every padding boundary, the decimal text of a field element against Python's str, the point text, the whole message of a
device proof and its (e1, e2) against tests/device_link_vectors.py, and the scalar stage.  The same program, built with the
address and undefined-behaviour sanitizers, answers the same requests on its own.  Pure CPU."""
import hashlib
import os
import random
import subprocess

import pytest

from conftest import ROOT
import device_link_vectors as D

o = D.o
Q, R = D.Q, D.R
SRC = os.path.join(ROOT, "tests", "cpp", "test_device_link.cpp")
IO = [D.COMMITTED, D.HIDDEN, D.COMMITTED, D.COMMITTED, D.REVEALED]


def hx(b):
    return bytes(b).hex() or "-"


def fe(v):
    return int(v).to_bytes(32, "little")


def ask_all(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = r.stdout.split()
    assert len(out) == len(lines) and "ERR" not in out, r.stdout[-2000:]
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("device_link") / "test_device_link")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", path, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


# ---- SHA-256 ------------------------------------------------------------------------------------------------------------------
def sha_messages():
    rng = random.Random(0x5A256)
    return [bytes(rng.randrange(256) for _ in range(n)) for n in list(range(201)) + [1000]]


def sha_lines():
    msgs = sha_messages()
    lines = ["sha " + hx(m) for m in msgs]
    want = [hashlib.sha256(m).hexdigest() for m in msgs]
    # the same digest from two runs, cut at every position of a 130-byte message: the block carried from one run to the next
    m = msgs[130]
    for cut in (0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 130):
        lines.append("sha2 %s %s" % (hx(m[:cut]), hx(m[cut:])))
        want.append(hashlib.sha256(m).hexdigest())
    return lines, want


def test_sha256_equals_hashlib_at_every_length(exe):
    lines, want = sha_lines()
    got = ask_all(exe, lines)
    for line, g, w in zip(lines, got, want):
        assert g == w, line[:80]


def test_sha256_known_answer(exe):
    """FIPS 180-4's "abc" """
    assert ask_all(exe, ["sha " + hx(b"abc")]) == ["ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"]


# ---- the text forms -----------------------------------------------------------------------------------------------------------
def dec_values():
    rng = random.Random(0xDEC)
    return [0, 1, 9, 10, 10**9 - 1, 10**9, 10**18, 10**27 - 1, R - 1, Q - 1] + [rng.randrange(1 << rng.randrange(1, 255)) for _ in range(20)]


def dec_lines():
    return ["dec " + hx(fe(v)) for v in dec_values()], [hx(("" if v == 0 else str(v)).encode()) for v in dec_values()]


def test_dec_equals_python_str(exe):
    lines, want = dec_lines()
    got = ask_all(exe, lines)
    for v, g, w in zip(dec_values(), got, want):
        assert g == w, v
    assert got[0] == "-"                       # zero is the empty string


def test_point_text(exe):
    """the generator is "(1, 2)", O is "infinity", and a random point "(x, y)": the digest over literal strings"""
    P = D.mul(o.G1_GEN, 0xC0FFEE)
    c0, hq = 12345, b"\x01\x02\x03"
    text = "12345" + "(1, 2)" + "infinity" + "(%d, %d)" % P
    want = hashlib.sha256(b"computing challenge for linking proof" + text.encode() + hq).hexdigest()
    line = " ".join(["digest", hx(fe(c0)), hx(o.g1_uncompressed(o.G1_GEN)), hx(o.g1_uncompressed(None)), hx(o.g1_uncompressed(P)), hx(hq)])
    assert ask_all(exe, [line]) == [want]
    assert D.message(c0, o.G1_GEN, None, P, hq) == b"computing challenge for linking proof" + text.encode() + hq


# ---- the whole message ----------------------------------------------------------------------------------------------------------
def digest_records():
    key = D.make_key(IO, 2, 3, 0xD1CE)
    rng = random.Random(0xD16E)
    return key, [D.random_record(key, rng, h_len=h) for h in (32, 0, 1, 64, 33)]


def digest_lines():
    key, recs = digest_records()
    lines = [" ".join(["digest", hx(fe(r.pi0_c)), hx(o.g1_uncompressed(r.com0)), hx(o.g1_uncompressed(r.com1)), hx(o.g1_uncompressed(r.comz)), hx(r.h_q)])
             for r in recs]
    return lines, [r.digest.hex() for r in recs]


def test_message_and_challenge_equal_the_restatement(exe):
    lines, want = digest_lines()
    assert ask_all(exe, lines) == want
    key, recs = digest_records()
    for r in recs:                             # and the restatement's own verifier accepts what its prover made
        assert D.verify(key, D.record_bytes(key, r)) == (D.ACCEPT, (D.ACCEPT, D.ACCEPT), r.digest)
        e1, e2 = D.e_of(r.digest)
        assert e1 < 1 << 128 and e2 < 1 << 128


# ---- the scalar stage -----------------------------------------------------------------------------------------------------------
def scalar_cases():
    """(name, fields, expected flags or None for 'malformed'): fields = m, c0, s0 x 4, c1, s1 x 3, e1, e2"""
    rng = random.Random(0x5CA1)
    s = lambda: rng.randrange(R)
    base = dict(m=s(), c0=s(), s0=[s(), s(), s(), s()], c1=s(), s1=[s(), s(), s()], e1=rng.getrandbits(128), e2=rng.getrandbits(128))
    eq = dict(base, s0=[base["s0"][0], base["s0"][1], base["s0"][0], base["s0"][3]])
    cases = [("eq_pos differs", base, 0), ("eq_pos holds", eq, 2), ("m = r - 1", dict(eq, m=R - 1), 2), ("e = 2^128 - 1", dict(eq, e1=(1 << 128) - 1, e2=(1 << 128) - 1), 2),
             ("everything zero", dict(m=0, c0=0, s0=[0] * 4, c1=0, s1=[0] * 3, e1=0, e2=0), 2)]
    for bad in (R, (1 << 256) - 1):
        for f in ("m", "c0", "c1"):
            cases.append(("%s = %x" % (f, bad), dict(eq, **{f: bad}), None))
        for j in range(4):
            cases.append(("s0[%d] = %x" % (j, bad), dict(eq, s0=[bad if i == j else v for i, v in enumerate(eq["s0"])]), None))
        for j in range(3):
            cases.append(("s1[%d] = %x" % (j, bad), dict(eq, s1=[bad if i == j else v for i, v in enumerate(eq["s1"])]), None))
    for f in ("m", "c0", "c1"):
        cases.append(("%s = r - 1" % f, dict(eq, **{f: R - 1}), 2))
    return cases


def scalar_lines():
    lines, want = [], []
    for _, c, flags in scalar_cases():
        e = int(c["e1"]).to_bytes(16, "little") + int(c["e2"]).to_bytes(16, "little")
        lines.append(" ".join(["scalars", hx(fe(c["m"])), hx(fe(c["c0"])), hx(b"".join(fe(x) for x in c["s0"])), hx(fe(c["c1"])),
                               hx(b"".join(fe(x) for x in c["s1"])), hx(e)]))
        if flags is None:
            want.append("1:" + bytes(96).hex())
        else:
            want.append("%d:%s" % (flags, b"".join(fe(c["c1"] * v % R) for v in (c["e1"], c["e2"], c["m"])).hex()))
    return lines, want


def test_scalar_stage(exe):
    lines, want = scalar_lines()
    got = ask_all(exe, lines)
    for (name, _, _), g, w in zip(scalar_cases(), got, want):
        assert g == w, name


def test_sanitized_build_answers_the_same(tmp_path):
    path = str(tmp_path / "test_device_link_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", path, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines, want = [], []
    for fn in (sha_lines, dec_lines, digest_lines, scalar_lines):
        a, b = fn()
        lines += a
        want += b
    assert ask_all(path, lines) == want
