"""The lazy 29-bit-limb arithmetic the hot kernels run (csrc/field29.hpp, csrc/curve29.hpp) checked on the HOST
against the saturated 8x32 Montgomery arithmetic (csrc/field.hpp, csrc/curve.hpp) — g++ build of
tests/cpp/test_field29.cpp and tests/cpp/test_ntt29_lazy.cpp — and its bound analysis (tools/bounds29.py).  Pure CPU."""
import os
import subprocess
import sys

from conftest import ROOT


def test_bounds_checker_passes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bounds29.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all bounds hold" in r.stdout
    # the transform's bounds, as csrc/wmap29.hip's comment and tests/cpp/test_ntt29_lazy.cpp quote them
    for line in ("ntt first group  packed < 5.29 N -> < 22.58 N", "ntt first   pass, 10 stages: values < 46.58 N",
                 "ntt first   pass, 11 stages: values < 49.58 N", "ntt strided pass,  6 stages: values < 21.00 N",
                 "ntt strided pass, 10 stages: values < 33.00 N", "ntt largest value in any plan (logn 0..28, both tiles): 49.58 N",
                 "weak_reduce v < 2^261", "k_fold29   products < 1.031 N, sums < 69.00 N for any number of terms",
                 "k_sell29   terms < 5.29 N, a piece < 42.32 N"):
        assert line in r.stdout, line


def test_field29_and_curve29_against_saturated_arithmetic(tmp_path):
    exe = str(tmp_path / "test_field29")
    src = os.path.join(ROOT, "tests", "cpp", "test_field29.cpp")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:]


def test_lazy_transform_steps_against_saturated_arithmetic(tmp_path):
    """weak_reduce at exact multiples of N and at its limits; one tile of k_ntt29_pass replayed on the host (both first-pass
    shapes, a 6- and a 10-stage strided shape, every STORE form) on lifted, equal, geometric and zero inputs"""
    exe = str(tmp_path / "test_ntt29_lazy")
    src = os.path.join(ROOT, "tests", "cpp", "test_ntt29_lazy.cpp")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:]
