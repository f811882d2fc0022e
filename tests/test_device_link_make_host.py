"""csrc/device_link_make.hpp on the HOST (g++ build of tests/cpp/test_device_link_make.cpp): the range stage of the 13 scalars,
the three response / recombination stages against Python integers, and a whole host-side proof - fixed-base walks through
host-built tables, the sums, the opening checks, both transcripts, the digest - against tests/device_link_vectors.py's `prove`.
The same program, built with the address and undefined-behaviour sanitizers, answers the same requests on its own.  Pure CPU."""
import os
import random
import subprocess

import pytest

from conftest import ROOT
import device_link_vectors as D

o = D.o
R = D.R
SRC = os.path.join(ROOT, "tests", "cpp", "test_device_link_make.cpp")
IO = [D.COMMITTED, D.HIDDEN, D.COMMITTED, D.COMMITTED, D.REVEALED]
OPEN = ("q0", "r0", "q1", "r1_orig")
RAND = ("z", "tz", "r1", "a", "b", "d", "n0", "n1", "n2")


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
    path = str(tmp_path_factory.mktemp("device_link_make") / "test_device_link_make")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", path, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def arrays(s):
    """a dict of the 13 scalars -> (openings 128 B, rand 288 B) as hex"""
    return hx(b"".join(fe(s[f]) for f in OPEN)), hx(b"".join(fe(s[f]) for f in RAND))


def scalars(rng, **kw):
    s = {f: rng.randrange(R) for f in OPEN + RAND}
    s.update(kw)
    return s


# ---- (i) the range checks ----------------------------------------------------------------------------------------------------
def range_lines():
    rng = random.Random(0x4A6E)
    base = scalars(rng)
    lines, want = ["range %s %s" % arrays(base)], ["1"]
    for f in OPEN + RAND:
        for v, ok in ((R - 1, "1"), (R, "0"), ((1 << 256) - 1, "0")):
            lines.append("range %s %s" % arrays(dict(base, **{f: v})))
            want.append(ok)
    lines.append("range %s %s" % arrays({f: 0 for f in OPEN + RAND}))
    want.append("1")
    return lines, want


def test_range_stage_on_each_of_the_13_scalars(exe):
    lines, want = range_lines()
    assert len(lines) == 2 + 13 * 3
    assert ask_all(exe, lines) == want


# ---- (ii), (iii), (iv) ---------------------------------------------------------------------------------------------------------
def stage_cases():
    """(name, scalars, c0, e1, e2, c1)"""
    rng = random.Random(0x57A6)
    c = lambda: rng.randrange(1 << 248)
    e = lambda: rng.getrandbits(128)
    top = (1 << 128) - 1
    cases = [("random %d" % i, scalars(rng), c(), e(), e(), c()) for i in range(4)]
    cases.append(("c = 0", scalars(rng), 0, e(), e(), 0))
    cases.append(("every secret zero", scalars(rng, q0=0, r0=0, q1=0, r1_orig=0, r1=0, z=0, tz=0), c(), e(), e(), c()))
    cases.append(("every nonce zero", scalars(rng, a=0, b=0, d=0, n0=0, n1=0, n2=0), c(), e(), e(), c()))
    cases.append(("e1 = e2 = 2^128 - 1", scalars(rng), c(), top, top, c()))
    cases.append(("everything r - 1", {f: R - 1 for f in OPEN + RAND}, R - 1, top, top, R - 1))
    s, e1, e2 = scalars(rng), e(), e()
    s["r0"] = -(s["r1"] * e1 + s["tz"] * e2) % R
    cases.append(("r comes out 0", s, c(), e1, e2, c()))
    s, e1, e2 = scalars(rng), e(), e()
    s["q0"] = -(s["q1"] * e1 + s["z"] * e2) % R
    cases.append(("m comes out 0", s, c(), e1, e2, c()))
    cases.append(("everything zero", {f: 0 for f in OPEN + RAND}, 0, 0, 0, 0))
    return cases


def stage_lines():
    lines, want = [], []
    for _, s, c0, e1, e2, c1 in stage_cases():
        ob, rb = arrays(s)
        m = (s["q0"] + s["q1"] * e1 + s["z"] * e2) % R
        r = (s["r0"] + s["r1"] * e1 + s["tz"] * e2) % R
        lines.append("pi0s %s %s %s" % (hx(fe(c0)), ob, rb))
        first = (s["a"] - c0 * s["q1"]) % R
        want.append(hx(b"".join(fe(v) for v in (first, (s["b"] - c0 * s["r1_orig"]) % R, first, (s["d"] - c0 * s["r1"]) % R))))
        lines.append("recombine %s %s %s" % (hx(e1.to_bytes(16, "little") + e2.to_bytes(16, "little")), ob, rb))
        want.append(hx(fe(m) + fe(r)))
        lines.append("pi1s %s %s %s" % (hx(fe(c1)), hx(fe(r)), rb))
        want.append(hx(b"".join(fe(v) for v in ((s["n0"] - c1 * r) % R, (s["n1"] - c1 * s["z"]) % R, (s["n2"] - c1 * s["tz"]) % R))))
    return lines, want


def test_response_and_recombination_stages(exe):
    lines, want = stage_lines()
    got = ask_all(exe, lines)
    names = [n for n, *_ in stage_cases() for _ in range(3)]
    for name, line, g, w in zip(names, lines, got, want):
        assert g == w, (name, line.split()[0])
    by_name = {n: i for i, (n, *_) in enumerate(stage_cases())}
    assert want[3 * by_name["r comes out 0"] + 1].endswith(bytes(32).hex())
    assert want[3 * by_name["m comes out 0"] + 1].startswith(bytes(32).hex())


# ---- a whole proof ---------------------------------------------------------------------------------------------------------------
def proof_records():
    key = D.make_key(IO, 2, 3, 0xD1CE)
    rng = random.Random(0x3A6E)
    out = []
    for h_len in (32, 0, 1, 64, 33):
        s = {f: rng.randrange(1, R) for f in OPEN + RAND}
        h_q = bytes(rng.randrange(256) for _ in range(h_len))
        out.append((s, D.prove(key, s["q0"], s["r0"], s["q1"], s["r1_orig"], s["r1"], s["z"], s["tz"], (s["a"], s["b"], s["d"]),
                               (s["n0"], s["n1"], s["n2"]), h_q)))
    return key, out


def proof_line(key, s, rec, **kw):
    pt = o.g1_uncompressed
    return " ".join(["prove", hx(pt(key.g)), hx(pt(key.gp)), hx(pt(key.h)), hx(kw.get("com0", pt(rec.com0))), hx(pt(rec.com1_orig)), *arrays(s),
                     hx(rec.h_q)])


def proof_answer(rec):
    pt = o.g1_uncompressed
    return ":".join(["1", hx(pt(rec.com1)), hx(pt(rec.comz)), hx(fe(rec.m)), hx(fe(rec.pi0_c)), hx(b"".join(fe(x) for x in rec.pi0_s)),
                     hx(fe(rec.pi1_c)), hx(b"".join(fe(x) for x in rec.pi1_s)), hx(rec.digest)])


def proof_lines():
    key, recs = proof_records()
    lines = [proof_line(key, s, rec) for s, rec in recs]
    want = [proof_answer(rec) for _, rec in recs]
    # an opening that does not open com0, and a com0 with both flag bits: malformed, every row zero
    s, rec = recs[0]
    zero = ":".join(["2"] + [bytes(n).hex() for n in (64, 64, 32, 32, 128, 32, 96, 32)])
    bad = bytearray(o.g1_uncompressed(rec.com0))
    bad[63] |= 0xC0
    lines += [proof_line(key, dict(s, q0=(s["q0"] + 1) % R), rec), proof_line(key, s, rec, com0=bytes(bad))]
    want += [zero, zero]
    return lines, want


def test_a_whole_host_side_proof_equals_the_restatement(exe):
    lines, want = proof_lines()
    got = ask_all(exe, lines)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, i
    key, recs = proof_records()
    assert [len(rec.h_q) for _, rec in recs] == [32, 0, 1, 64, 33]
    for _, rec in recs:                        # and the restatement's own verifier accepts what its prover made
        assert D.verify(key, D.record_bytes(key, rec)) == (D.ACCEPT, (D.ACCEPT, D.ACCEPT), rec.digest)


def test_sanitized_build_answers_the_same(tmp_path):
    path = str(tmp_path / "test_device_link_make_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", path, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines, want = [], []
    for fn in (range_lines, stage_lines, proof_lines):
        a, b = fn()
        lines += a
        want += b
    assert ask_all(path, lines) == want
