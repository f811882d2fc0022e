"""The link between a showing's two halves on the HOST (g++ build of tests/cpp/test_show_link.cpp): csrc/show_link.hpp's
shift_commitment and shift_opening against oracle/bn254_oracle.py, and csrc/merlin.hpp's one-text DLogPoK transcript
(ml_dlog_shape_challenge, what k_show_challenge runs per lane) against the pure-Python Merlin of tests/merlin_vectors.py and
against the host's existing ml_dlog_challenge, byte for byte.  The same program, built with the address and
undefined-behaviour sanitizers, answers the same requests on its own.  Pure CPU."""
import os
import random
import subprocess

import pytest

from conftest import ROOT
import merlin_vectors as MV
import range_vectors as RV

o = RV.o
R = o.R
SRC = os.path.join(ROOT, "tests", "cpp", "test_show_link.cpp")


def hx(b):
    return bytes(b).hex() or "-"


def pt(P):
    """x ‖ y, zeros for O"""
    return bytes(64) if P is None else P[0].to_bytes(32, "little") + P[1].to_bytes(32, "little")


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
    path = str(tmp_path_factory.mktemp("show_link") / "test_show_link")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", path, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


# ---- the transcript --------------------------------------------------------------------------------------------------------
def transcript_cases():
    """(context or None, shape): the issue's shapes against every context length around the STROBE rate of 166"""
    rng = random.Random(0x5107)
    ctx = lambda n: bytes(rng.randrange(256) for _ in range(n))
    cases = []
    for shape in ([1], [2, 2, 5]):
        for context in [None] + [ctx(n) for n in (0, 1, 165, 166, 167, 1000)]:
            cases.append((context, shape))
    return cases


def transcript_request(cmd, context, shape, rng):
    rnd = lambda: bytes(rng.randrange(256) for _ in range(32))
    st = [([rnd() for _ in range(nb)], rnd(), rnd()) for nb in shape]
    line = " ".join([cmd, "none" if context is None else hx(context), ",".join(map(str, shape)), hx(b"".join(b for s in st for b in s[0])),
                     hx(b"".join(s[1] for s in st)), hx(b"".join(s[2] for s in st))])
    return line, MV.to_scalar_bytes(MV.dlog_challenge(context, st)).hex()


def transcript_lines(cmd):
    rng = random.Random(0xD106)
    return [transcript_request(cmd, context, shape, rng) for context, shape in transcript_cases()]


def test_one_text_transcript_equals_the_python_merlin(exe):
    reqs = transcript_lines("dlog1")
    got = ask_all(exe, [line for line, _ in reqs])
    for (context, shape), g, (_, want) in zip(transcript_cases(), got, reqs):
        assert g == want, (None if context is None else len(context), shape)


def test_one_text_transcript_equals_the_host_transcript(exe):
    """the same operands through ml_dlog_challenge (MerlinTranscript): what cg_dlog_challenge_batch runs"""
    new, old = transcript_lines("dlog1"), transcript_lines("dlog0")
    assert [w for _, w in new] == [w for _, w in old]
    assert ask_all(exe, [line for line, _ in new]) == ask_all(exe, [line for line, _ in old])


def test_known_answers_of_the_shape(exe):
    lines, want = [], []
    for context, shape, c in MV.KAT_DLOG:
        st = MV.kat_statements(shape)
        lines.append(" ".join(["dlog1", "none" if context is None else hx(context), ",".join(map(str, shape)), hx(b"".join(b for s in st for b in s[0])),
                               hx(b"".join(s[1] for s in st)), hx(b"".join(s[2] for s in st))]))
        want.append(c + "00")
    assert ask_all(exe, lines) == want


# ---- the link ----------------------------------------------------------------------------------------------------------------
def link_cases():
    """(name, base scalar b, committed scalar or None for O, t): base = b G, committed = cc G, expected (cc - t b) G"""
    rng = random.Random(0x11E4)
    b, cc = rng.randrange(1, R), rng.randrange(1, R)
    t64 = rng.getrandbits(64) | (1 << 63)
    t = rng.randrange(1, R)
    return [("t = 0", b, cc, 0), ("t = 1", b, cc, 1), ("t = r - 1", b, cc, R - 1), ("a 64-bit t", b, cc, t64), ("a full-width t", b, cc, t),
            ("committed = t base: O", b, t * b % R, t), ("committed = -t base: a doubling", b, -t * b % R, t),
            ("committed = t base, 64-bit t: O", b, t64 * b % R, t64), ("committed = O", b, None, t), ("committed = O, t = 0", b, None, 0)]


def link_lines():
    lines, want = [], []
    for _, b, cc, t in link_cases():
        lines.append(" ".join(["shift", hx(pt(RV.g1(b))), hx(pt(None if cc is None else RV.g1(cc))), hx(fe(t))]))
        want.append(pt(RV.g1(((0 if cc is None else cc) - t * b) % R)).hex())
    return lines, want


def test_shift_commitment_equals_the_oracle(exe):
    lines, want = link_lines()
    got = ask_all(exe, lines)
    for (name, _, _, _), g, w in zip(link_cases(), got, want):
        assert g == w, name
    names = [c[0] for c in link_cases()]
    assert want[names.index("committed = t base: O")] == bytes(64).hex()          # O is a legal ped_com
    assert want[names.index("committed = -t base: a doubling")] != bytes(64).hex()


def opening_cases():
    rng = random.Random(0x09E2)
    m, t = sorted(rng.randrange(R) for _ in range(2))
    return [(m, t), (t, m), (0, 1), (0, R - 1), (R - 1, R - 1), (5, 0), (1 << 31, (1 << 64) - 1)]


def test_shift_opening_wraps_mod_r(exe):
    cases = opening_cases()
    assert any(m < t for m, t in cases)
    got = ask_all(exe, ["open %s %s" % (hx(fe(m)), hx(fe(t))) for m, t in cases])
    assert got == [fe((m - t) % R).hex() for m, t in cases]
    assert ask_all(exe, ["below " + hx(fe(v)) for v in (0, R - 1, R, R + 1, (1 << 256) - 1)]) == ["1", "1", "0", "0", "0"]


def test_sanitized_build_answers_the_same(tmp_path):
    path = str(tmp_path / "test_show_link_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", path, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    reqs = transcript_lines("dlog1")
    lines, want = link_lines()
    cases = opening_cases()
    got = ask_all(path, [line for line, _ in reqs] + lines + ["open %s %s" % (hx(fe(m)), hx(fe(t))) for m, t in cases])
    assert got == [w for _, w in reqs] + want + [fe((m - t) % R).hex() for m, t in cases]
