"""The latency arrangement of the range-proof verifier (cg_range_vk_set_latency_mode; csrc/pairing_team.hpp,
k_rv_lone_miller / k_rv_lone_final in csrc/rangeverify.hip): the pairing of each showing on one workgroup.  Every test
compares three things with each other: the trapdoor restatement of tests/range_verify_vectors.py (route (a)), the wide
arrangement, and the latency arrangement on the same handle - verdicts and k_out bytes.  n_bits = 4 throughout."""
import random

import numpy as np
import pytest

import range_vectors as RV
import range_verify_vectors as V

pytestmark = pytest.mark.gpu

R = V.R
ACCEPT, REJECT, MALFORMED = V.ACCEPT, V.REJECT, V.MALFORMED
INVALID_ARGUMENT = -1
CHUNK = 1 << 15                      # showings per launch set (csrc/rangeverify.hip, RVCHUNK)
unc = V.unc


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


def load(cc, K, **kw):
    gpu = cc.RangeVerifyingKey(V.vk_bytes(K, **kw), K.n_bits)
    return gpu, gpu.add_bases(*[unc(P) for P in V.bases_of()])


@pytest.fixture(scope="module")
def vk4(cc):
    K = RV.key(4)
    gpu, slot = load(cc, K)
    yield K, gpu, slot
    gpu.close()


@pytest.fixture(scope="module")
def rows4(vk4):
    """the rows every test draws from, with route (a)'s verdict and k bytes, computed once"""
    K = vk4[0]
    rng = random.Random(5000)
    bases = V.bases_of()
    named = [("valid %d" % i, V.valid_row(K, bases, rng)[0]) for i in range(3)]
    named += [("forged %d" % i, V.forged_row(K, rng)) for i in range(2)]
    good, bad = V.total_w_zero_rows(K, rng)
    named += [("total_w = O, total_c = O", good), ("total_w = O, total_c != O", bad), ("all infinity", V.all_infinity_row())]
    x = named[0][1]
    named += [("eval_gw off", x.with_item("evals", 1, x.evals[1] ^ 1)), ("rho = 1", x.but(rho=1)),
              ("a forged row's eval_w^ off", named[3][1].with_item("evals", 2, named[3][1].evals[2] ^ 1))]
    rows = [x for _, x in named]
    wants = [V.expected(K, bases, x) for x in rows]
    assert [w[0] for w in wants] == [ACCEPT] * 6 + [REJECT, ACCEPT, REJECT, MALFORMED, REJECT]
    return [n for n, _ in named], rows, wants


def both(cc, gpu, slot, rows, wants, pok=True):
    a = V.pack(rows)
    for mode in (False, True):
        gpu.set_latency(mode)
        if pok:
            verdicts, k = cc.Groth16.range_verify_batch_packed(gpu, slot, *a)
            assert [k[i].tobytes() for i in range(len(rows))] == [w[1] for w in wants], mode
        else:
            verdicts, k = cc.Groth16.range_verify_batch_packed(gpu, slot, None, *a[1:9])
            assert k is None
        assert list(verdicts) == [w[0] for w in wants], (mode, list(verdicts))
    gpu.set_latency(False)


def test_the_setters_exist(cc, vk4):
    L = cc.lib()
    assert hasattr(L, "cg_range_vk_set_latency_mode")
    gpu = vk4[1]
    for on in (1, 0):
        assert L.cg_range_vk_set_latency_mode(gpu._h, on) == 0
    for bad in (2, -1, 1 << 20):
        assert L.cg_range_vk_set_latency_mode(gpu._h, bad) == INVALID_ARGUMENT, bad
        assert b"latency mode" in L.cg_last_error()
    assert L.cg_range_vk_set_latency_mode(None, 1) == INVALID_ARGUMENT


@pytest.mark.parametrize("n", [1, 3])
def test_valid_and_forged_rows(cc, vk4, rows4, n):
    K, gpu, slot = vk4
    _, rows, wants = rows4
    both(cc, gpu, slot, rows[:n], wants[:n])                     # valid rows
    both(cc, gpu, slot, rows[3:3 + n], wants[3:3 + n])           # forged rows, then total_w = O


def test_every_kind_in_one_batch_and_alone(cc, vk4, rows4):
    """total_w = O drops the pair (-total_w, beta_h), all infinity drops both: f = 1 from a workgroup that ran no step"""
    K, gpu, slot = vk4
    names, rows, wants = rows4
    both(cc, gpu, slot, rows, wants)
    for name in ("total_w = O, total_c = O", "total_w = O, total_c != O", "all infinity", "rho = 1"):
        i = names.index(name)
        both(cc, gpu, slot, rows[i:i + 1], wants[i:i + 1])


def test_a_key_whose_beta_h_is_infinity(cc, rows4):
    K = RV.key(4)
    names, rows, _ = rows4
    pick = [rows[names.index(n)] for n in ("valid 0", "all infinity", "total_w = O, total_c = O", "total_w = O, total_c != O")]
    wants = [V.expected(K, V.bases_of(), x, beta_h_inf=True) for x in pick]
    assert [w[0] for w in wants] == [REJECT, ACCEPT, ACCEPT, REJECT]
    gpu, slot = load(cc, K, beta_h_inf=True)
    try:
        both(cc, gpu, slot, pick, wants)
        both(cc, gpu, slot, pick[:1], wants[:1])
    finally:
        gpu.close()


def test_without_a_dleq(cc, vk4, rows4):
    K, gpu, slot = vk4
    names, rows, _ = rows4
    pick = [rows[names.index(n)] for n in ("valid 1", "eval_gw off", "rho = 1")]
    wants = [V.expected(K, V.bases_of(), x, pok=False) for x in pick]
    assert [w[0] for w in wants] == [ACCEPT, REJECT, MALFORMED]
    both(cc, gpu, slot, pick, wants, pok=False)
    both(cc, gpu, slot, pick[:1], wants[:1], pok=False)


def test_a_batch_of_one_chunk_plus_one(cc, vk4, rows4):
    K, gpu, slot = vk4
    names, rows, wants = rows4
    idx = [names.index(n) for n in ("valid 2", "eval_gw off", "forged 0", "rho = 1", "all infinity")]
    kinds, kw = [rows[i] for i in idx], [wants[i] for i in idx]
    n = CHUNK + 1
    a = [np.tile(np.frombuffer(b, np.uint8).reshape(5, -1), (n // 5 + 1, 1))[:n] for b in V.pack(kinds)]
    for mode in (False, True):
        gpu.set_latency(mode)
        verdicts, k = cc.Groth16.range_verify_batch_packed(gpu, slot, *a)
        assert verdicts.shape == (n,) and k.shape == (n, 2, 32)
        for i in range(5):
            assert (verdicts[i::5] == kw[i][0]).all(), (mode, i)
            assert (k[i::5].reshape(-1, 64) == np.frombuffer(kw[i][1], np.uint8)).all(), (mode, i)
    gpu.set_latency(False)


def test_mode_switching_between_calls(cc, vk4, rows4):
    """on, off, on on one handle between calls of different n: the same bytes each time"""
    K, gpu, slot = vk4
    _, rows, wants = rows4
    for mode, n in ((True, 3), (False, 11), (True, 1), (True, 11), (False, 2), (True, 2)):
        gpu.set_latency(mode)
        verdicts, k = cc.Groth16.range_verify_batch_packed(gpu, slot, *V.pack(rows[:n]))
        assert list(verdicts) == [w[0] for w in wants[:n]], (mode, n)
        assert [k[i].tobytes() for i in range(n)] == [w[1] for w in wants[:n]], (mode, n)
    gpu.set_latency(False)
    group_ms, pairing_ms = gpu.last_kernel_ms()
    assert group_ms > 0 and pairing_ms > 0
