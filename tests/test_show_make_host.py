"""The two pieces of creating a whole showing that host and device share, on the HOST (g++ build of
tests/cpp/test_show_make.cpp): csrc/show_make.hpp's response row s = nonce - c secret mod r against Python integers, and the
place of a range link's opening (m, r) in a showing's `inputs` and `rand` against a restatement of the order in which
include/crescent_gpu.h lays the random scalars out (r1, r2, the r_i, z, the nonces).  The same program, built with the
address and undefined-behaviour sanitizers, answers the same requests on its own.  Pure CPU."""
import os
import random
import subprocess

import pytest

from conftest import ROOT
import range_vectors as RV
import show_vectors as S

R = RV.o.R
SRC = os.path.join(ROOT, "tests", "cpp", "test_show_make.cpp")
COM, HID, REV = S.COMMITTED, S.HIDDEN, S.REVEALED
LAYOUTS = {"one": [COM, REV, HID], "mdl": [COM, HID, COM, REV]}


def fe(v):
    return int(v).to_bytes(32, "little").hex()


def ask_all(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = r.stdout.split()
    assert len(out) == len(lines) and "ERR" not in out, r.stdout[-2000:]
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("show_make") / "test_show_make")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", path, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def row_cases():
    """(name, c, secret, nonce)"""
    rng = random.Random(0x5E5B)
    c, x, k = (rng.randrange(1, R) for _ in range(3))
    small_k = rng.randrange(1, 1 << 64)
    cases = [("c = 0", 0, x, k), ("secret = 0", c, 0, k), ("nonce = 0", c, x, 0), ("nonce < c secret: wraps", c, x, small_k),
             ("all three r - 1", R - 1, R - 1, R - 1), ("a 248-bit c", c >> 6, x, k), ("everything 0", 0, 0, 0), ("c = 1, secret = nonce", 1, x, x)]
    assert c * x % R > small_k
    cases += [("random %d" % i, rng.randrange(R), rng.randrange(R), rng.randrange(R)) for i in range(16)]
    return cases


def row_lines():
    cases = row_cases()
    return ["row %s %s %s" % (fe(c), fe(x), fe(k)) for _, c, x, k in cases], [fe((k - c * x) % R) for _, c, x, k in cases]


def test_response_row_equals_python_integers(exe):
    lines, want = row_lines()
    got = ask_all(exe, lines)
    for (name, _, _, _), g, w in zip(row_cases(), got, want):
        assert g == w, name
    names = [c[0] for c in row_cases()]
    assert want[names.index("c = 1, secret = nonce")] == fe(0)


def opening_cases():
    """(layout, showing p, link's committed index) -> the request and the indices, from the header's order of `rand`"""
    out = []
    for name, io in LAYOUTS.items():
        com = [i for i, t in enumerate(io) if t == COM]
        n_hid = io.count(HID)
        n_resp = 2 * len(com) + n_hid + 1
        names = ["r1", "r2"] + ["r_%d" % ci for ci in range(len(com))] + ["z"] + ["nonce_%d" % t for t in range(n_resp)]
        n_rand = len(names)
        assert n_rand == 3 + len(com) + n_resp
        for p in (0, 1, 64, 4097, 32768, (1 << 32) + 5):
            for ci, pos in enumerate(com):
                out.append(("at %d %d %d %d %d" % (p, len(io), n_rand, pos, ci), "%d,%d" % (p * len(io) + pos, p * n_rand + names.index("r_%d" % ci)),
                            (name, p, ci)))
    return out


def test_link_opening_lies_where_the_header_says(exe):
    cases = opening_cases()
    assert {c[2][0] for c in cases} == {"one", "mdl"} and any(c[2][2] == 1 for c in cases)
    got = ask_all(exe, [line for line, _, _ in cases])
    for (_, want, what), g in zip(cases, got):
        assert g == want, what


def test_sanitized_build_answers_the_same(tmp_path):
    path = str(tmp_path / "test_show_make_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", path, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines, want = row_lines()
    cases = opening_cases()
    assert ask_all(path, lines + [line for line, _, _ in cases]) == want + [w for _, w, _ in cases]
