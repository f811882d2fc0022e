"""The per-row predicate of the witness check (csrc/satcheck.hpp: is <A_i,w>·<B_i,w> = <C_i,w> mod r, on the lazy packed
operands the sparse product leaves) on the HOST against Python integers - g++ build of tests/cpp/test_satcheck.cpp.
Pure CPU.  Operands are x·R' (R' = 2^261) in ANY representative below 2^256: the kernel must answer for the class."""
import os
import random
import subprocess

from conftest import ROOT

N = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
RP = 1 << 261
RP_INV = pow(RP, -1, N)
CAP = 1 << 256          # what the 32-byte packed form can hold (< 5.3 N); k_sell29 leaves < 3N, k_w_to29 < 2N


def _reps(x_mont):
    """every representative of the class of x_mont the packed form can hold"""
    x = x_mont % N
    return [x + k * N for k in range(6) if x + k * N < CAP]


def _rows():
    rng = random.Random(20261016)
    rows = []          # (A, B, C) packed integers

    def mont(x):
        return x * RP % N

    def add(a, b, c, ka=None, kb=None, kc=None):
        ra, rb, rc = _reps(mont(a)), _reps(mont(b)), _reps(mont(c))
        rows.append((ra[ka % len(ra)] if ka is not None else rng.choice(ra), rb[kb % len(rb)] if kb is not None else rng.choice(rb),
                     rc[kc % len(rc)] if kc is not None else rng.choice(rc)))

    # random satisfied and unsatisfied rows, random representatives
    for _ in range(1500):
        a, b = rng.randrange(N), rng.randrange(N)
        add(a, b, a * b % N)
        add(a, b, rng.randrange(N))
    # the edges: operands 0 and N-1, every representative up to 3N (and the few above it the form still holds)
    for a in (0, 1, N - 1):
        for b in (0, 1, N - 1):
            for ka in range(5):
                for kb in range(5):
                    for kc in range(5):
                        add(a, b, a * b % N, ka, kb, kc)                  # a·b and c as DIFFERENT representatives of one class
                        add(a, b, (a * b + 1) % N, ka, kb, kc)            # c off by exactly +1
                        add(a, b, (a * b - 1) % N, ka, kb, kc)            # ... and -1
    # c off by ±1 and by ±N∓1 as PACKED integers (the R' form values themselves), around every representative
    for _ in range(300):
        a, b = rng.randrange(N), rng.randrange(N)
        c_m = mont(a * b % N)
        for base in _reps(c_m):
            for off in (0, 1, -1, N - 1, -(N - 1), N, -N):
                C = base + off
                if 0 <= C < CAP:
                    rows.append((rng.choice(_reps(mont(a))), rng.choice(_reps(mont(b))), C))
    # the largest operands the form holds
    rows.append((CAP - 1, CAP - 1, (CAP - 1) * (CAP - 1) * RP_INV % N))
    rows.append((CAP - 1, CAP - 1, ((CAP - 1) * (CAP - 1) * RP_INV + 1) % N))
    rows.append((CAP - 1, CAP - 1, CAP - 1))
    return rows


def test_row_predicate_against_python_integers(tmp_path):
    exe = str(tmp_path / "test_satcheck")
    src = os.path.join(ROOT, "tests", "cpp", "test_satcheck.cpp")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = _rows()
    text = "".join("%064x %064x %064x\n" % row for row in rows)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = r.stdout.split("\n")
    assert lines[len(rows)] == "DONE" and len(lines) >= len(rows) + 1
    n_ok = n_bad = 0
    for (A, B, Cv), line in zip(rows, lines):
        got_ok, ga, gb, gc = line.split()
        # truth: A = a·R', B = b·R', C = c·R' (mod N)  =>  a·b = c  <=>  A·B = C·R' (mod N)
        want_ok = (A * B - Cv * RP) % N == 0
        assert int(got_ok) == int(want_ok), (hex(A), hex(B), hex(Cv), want_ok)
        assert int(ga, 16) == A * RP_INV % N and int(gb, 16) == B * RP_INV % N and int(gc, 16) == Cv * RP_INV % N
        n_ok += want_ok
        n_bad += not want_ok
    assert n_ok > 3000 and n_bad > 5000          # both answers are exercised
