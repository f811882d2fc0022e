"""Every closed form of tests/transform_vectors.py against the Python oracle (logn <= 6) and oracle/cpu_ref.c (logn 12), and
the two vanishing-quotient circuits against cpu_ref.witness_map: the GPU file (tests/test_gpu_transform_values.py) is never
the first to evaluate a formula.  Pure CPU."""
import numpy as np
import pytest

import bn254_oracle as o
import cpu_ref
import transform_vectors as T

R = o.R


def _ints(b):
    raw = np.ascontiguousarray(b, np.uint8).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _oracle(mode, v):
    inverse, coset = mode
    if not inverse:
        return o.coset_fft(v) if coset else o.fft(v)
    return o.coset_ifft(v) if coset else o.ifft(v)


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
@pytest.mark.parametrize("logn", [0, 1, 2, 3, 6])
def test_closed_forms_equal_the_python_oracle(mode, logn):
    n = 1 << logn
    wrong = []
    for label, x, want in T.families(mode, logn):
        got = _oracle(mode, _ints(x))
        if got != _ints(want):
            wrong.append(label)
        if label.startswith("geometric"):
            assert sum(1 for v in _ints(want) if v) == 1 and sum(1 for v in got if v) == 1, label     # zero everywhere but one
    assert not wrong, wrong
    assert len(list(T.families(mode, logn))) == 3 * (len(T.k0_choices(n)) + len(T.delta_choices(n))) + 1


@pytest.mark.parametrize("mode", T.MODES, ids=T.MODE_IDS)
def test_closed_forms_equal_cpu_ref_at_2_12(mode):
    wrong = []
    for label, x, want in T.families(mode, 12):
        T.report(wrong, label, cpu_ref.ntt(x, inverse=mode[0], coset=mode[1], nthreads=4), want)
    assert not wrong, wrong


def test_mismatch_report_names_every_differing_element():
    a = np.zeros(8 * 32, np.uint8)
    b = a.copy()
    b[3 * 32] = 1
    b[7 * 32 + 31] = 9
    assert list(T.mismatches(a, b)) == [3, 7]
    wrong = []
    T.report(wrong, "x", a, b)
    T.report(wrong, "same", a, a)
    assert len(wrong) == 1 and wrong[0][0] == "x" and wrong[0][1] == 2 and wrong[0][2][0] == (3, "0x0", "0x1")


@pytest.mark.parametrize("D", [1 << 5, 1 << 10])
def test_b_and_c_vanish_gives_zero_h_and_zero_coset_values(D):
    c = T.b_and_c_vanish(D)
    assert c.D == D
    h = cpu_ref.witness_map(c.mats, c.l, c.m, c.M, c.w, nthreads=4)
    assert h.size == D * 32 and not h.any()
    a = c.side_values(0)
    assert (a[:c.m + c.l].reshape(-1, 32).any(axis=1)).all()                # a dense and non-zero
    assert not c.side_values(1).any() and not c.side_values(2).any()
    va, vb = c.coset_sides(nthreads=4)
    assert all(va) and not any(vb)
    if D == 32:
        rows = [[[(int.from_bytes(m.coeff[32 * t:32 * t + 32].tobytes(), "little"), int(m.col[t]))
                  for t in range(int(m.row_ptr[i]), int(m.row_ptr[i + 1]))] for i in range(c.m)] for m in c.mats]
        assert o.witness_map_from_matrices(rows, c.l, c.m, _ints(c.w)) == [0] * D


@pytest.mark.parametrize("beta", [1, R - 1, 0x1234567890abcdef1234567890abcdef1234567890abcdef], ids=["one", "r-1", "other"])
def test_constant_sides_gives_zero_h_and_dense_coset_values(beta):
    D = 1 << 10
    c = T.constant_sides(D, beta)
    assert c.D == D
    h = cpu_ref.witness_map(c.mats, c.l, c.m, c.M, c.w, nthreads=4)
    assert not h.any()
    one = T.fr_bytes(1)
    assert (c.side_values(0) == one).all()                                  # a = 1 on all D points
    assert c.side_values(1).tobytes() == c.side_values(2).tobytes()         # b = c
    va, vb = c.coset_sides(nthreads=4)
    vinv = T.inv(pow(T.G, D, R) - 1)
    assert va == [vinv] * D and all(vb)
