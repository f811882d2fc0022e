"""Verifying range proofs without a GPU: the restatement of tests/range_verify_vectors.py against itself (its trapdoor route
and its pairing route agree; what range_vectors.prove makes it accepts, with the k points the prover absorbed; a flipped
evaluation, random_v or s_13 it rejects), csrc/rangeverify.hpp on the HOST (g++ build of tests/cpp/test_rangeverify.cpp)
against the restatement's merged scalars and bits, the errors of cg_range_vk_load and the null-handle errors of the other
entries - reported before any HIP call, so they carry their own codes on a box with no device - and the entries declared,
exported and bound.  (A handle needs a device: the null arrays, the unknown slot and n = 0 of cg_range_verify_batch are in
tests/test_gpu_range_verify.py.)"""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import range_vectors as RV
import range_verify_vectors as V

R = V.R
OK, INVALID_ARGUMENT, PARSE = 0, -1, -7


@pytest.fixture(scope="module")
def proved():
    rng = random.Random(31)
    K = RV.key(4)
    bases = V.bases_of()
    row, made = V.valid_row(K, bases, rng)
    return K, bases, row, made


def test_the_two_routes_agree(proved):
    """an accept, a reject, the cancelling-randomizer pair and the all-infinity row, each by the trapdoor and by the pairing"""
    K, bases, row, _ = proved
    rng = random.Random(32)
    keep, lose = V.cancelling_rows(row, rng.randrange(R))
    tw0, tw0_bad = V.total_w_zero_rows(K, rng)
    rows = [(row, True), (row.with_item("evals", 0, row.evals[0] ^ 1), False), (keep, True), (lose, False), (V.all_infinity_row(), True),
            (tw0, True), (tw0_bad, False)]
    for i, (x, want) in enumerate(rows):
        tc, tw = V.totals(K, 4, x, V.parse(x))
        assert V.pairing_by_trapdoor(K, tc, tw) == want, i
        assert V.pairing_by_ark(K, tc, tw) == want, i
    # the key's h may be any non-zero multiple of the generator, and beta_h = O leaves e(total_c, h) alone
    tc, tw = V.totals(K, 4, row, V.parse(row))
    assert V.pairing_by_ark(K, tc, tw, h_scalar=12345)
    assert not V.pairing_by_ark(K, tc, tw, beta_h_inf=True) and not V.pairing_by_trapdoor(K, tc, tw, beta_h_inf=True)
    assert V.pairing_by_ark(K, None, None, beta_h_inf=True) and V.pairing_by_ark(K, None, tw, beta_h_inf=True)
    # the sign: with total_w in place of -total_w the product is not one
    h, beta_h = V.key_g2(K)
    f = V.AF.multi_miller_loop([(tw, V.AF.g2_prepare(beta_h)), (tc, V.AF.g2_prepare(h))])
    assert V.AF.final_exponentiation(f) != V.o._f12_one()


def test_proofs_of_the_prover_are_accepted_with_its_k(proved):
    K, bases, row, made = proved
    verdict, k = V.expected(K, bases, row)
    assert verdict == V.ACCEPT and k == RV.expected_commit(made)[2][64:]
    assert V.expected(K, bases, row, pok=False) == (V.ACCEPT, None)
    # the verifier of range_vectors.py, written before this one, agrees on the same bytes
    proof = RV.ark_bytes(row.com_f, row.com_g, V.fes(row.evals), b"".join(W + V.fe(v) for W, v in zip(row.W, row.vs)), row.com_q, row.pok_c, row.s)
    assert RV.verify(K, bases, V.rd_g1_checked(row.ped_com)[1], proof, row.c, row.rho, k)


def test_a_flipped_eval_random_v_or_s13_is_rejected(proved):
    K, bases, row, _ = proved
    for j in range(3):
        assert V.expected(K, bases, row.with_item("evals", j, row.evals[j] ^ 1))[0] == V.REJECT, j
        assert V.expected(K, bases, row.with_item("vs", j, row.vs[j] ^ 1))[0] == V.REJECT, j
    bad = row.with_item("s", 5, row.s[5] ^ 1)
    assert V.expected(K, bases, bad)[0] == V.REJECT and V.expected(K, bases, bad, pok=False)[0] == V.ACCEPT
    assert V.expected(K, bases, row.but(c=row.c ^ 1))[0] == V.REJECT and V.expected(K, bases, row.but(rho=row.rho ^ 1))[0] == V.REJECT


def test_forged_proofs_are_accepted_under_any_randomizers():
    K = RV.key(4)
    rng = random.Random(33)
    w = V.o.root_of_unity(4)
    for kw in ({}, {"rho": w}, {"rho": 0}, {"c": 0}, {"a_g": 0}, {"r1": 0, "r2": 0}, {"r1": 2 ** 128 - 1, "r2": 2 ** 128 - 1}):
        x = V.forged_row(K, rng, **kw)
        assert V.expected(K, V.bases_of(), x)[0] == V.ACCEPT, kw
        assert V.expected(K, V.bases_of(), x.with_item("vs", 2, x.vs[2] ^ 1))[0] == (V.ACCEPT if kw.get("r2") == 0 else V.REJECT), kw


# ---- the scalar stage on the host ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rangeverify") / "test_rangeverify")
    src = os.path.join(ROOT, "tests", "cpp", "test_rangeverify.cpp")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(n, x, pok=True):
        line = "%d %s %s %s %s %s" % (n.bit_length() - 1, V.fes(x.evals).hex(), V.fes(x.vs).hex(), V.fe(x.c).hex(), V.fe(x.rho).hex(),
                                      (x.r1.to_bytes(16, "little") + x.r2.to_bytes(16, "little")).hex())
        if pok:
            line += " %s %s" % (V.fe(x.pok_c).hex(), V.fes(x.s).hex())
        p.stdin.write(line + "\n")
        p.stdin.flush()
        out = p.stdout.readline().strip()
        assert out != "ERR", line[:60]
        return out
    yield ask
    p.stdin.close()
    p.wait(timeout=30)


def want_line(n, x, pok=True):
    return "%d %d %s" % (V.identity_holds(n, x), (not pok) or x.s[0] == x.s[5], V.fes(V.merged_scalars(n, x)).hex())


def scalar_row(rng, **kw):
    """a row of scalars alone (the points are not read by the scalar stage); the identity holds unless kw breaks it"""
    K = RV.key(4)      # only its trapdoor is used: the forger's eval_w^ does not depend on the key's size
    return V.forged_row(K, rng, **kw)


def identity_row(n, rng, **kw):
    """scalars whose eval_w^ satisfies the identity for a domain of n"""
    x = scalar_row(rng, **kw)
    wl = pow(V.o.root_of_unity(n), n - 1, R)
    q_coeff, f_coeff = V.coeffs(n, x.rho)
    eg, egw = x.evals[:2]
    d = (eg - 2 * egw) % R
    ew = (eg * f_coeff + x.c * eg * (1 - eg) % R * q_coeff % R * V.inv((x.rho - wl) % R) + x.c * x.c * d % R * (1 - d) % R * (x.rho - wl)) % R
    return x.with_item("evals", 2, ew)


@pytest.mark.parametrize("n", [2, 4, 32])
def test_scalar_stage_matches_the_restatement(tool, n):
    rng = random.Random(40 + n)
    w = V.o.root_of_unity(n)
    wl = pow(w, n - 1, R)
    top = 2 ** 128 - 1
    cases = [{}, {"rho": 0}, {"c": 0}, {"r1": 0, "r2": 0}, {"r1": top, "r2": top}, {"r1": top, "r2": 0}, {"eval_g": 0, "eval_gw": 0},
             {"eval_g": R - 1, "eval_gw": R - 1, "vs": [R - 1] * 3, "c": R - 1, "rho": R - 2}]
    if n > 2:
        cases.append({"rho": w})                                  # rho^n = 1 and not malformed: q_coeff = f_coeff = 0
    for kw in cases:
        x = identity_row(n, rng, **kw)
        assert V.identity_holds(n, x)
        for pok in (True, False):
            assert tool(n, x, pok) == want_line(n, x, pok), (kw, pok)
        if kw.get("rho") == w:
            assert V.merged_scalars(n, x)[1:3] == [0, 0]
        broken = x.with_item("evals", rng.randrange(3), rng.randrange(R))
        assert tool(n, broken) == want_line(n, broken) and tool(n, broken).startswith("0 1 "), kw
        off = x.with_item("s", 5, (x.s[5] + 1) % R)
        assert tool(n, off).startswith("1 0 ") and tool(n, off, False).startswith("1 1 "), kw
    x = identity_row(n, rng)
    for rho in {1, wl}:
        assert tool(n, x.but(rho=rho)) == "MALFORMED" and tool(n, x.but(rho=rho), False) == "MALFORMED", rho
    for j in range(3):
        assert tool(n, x.with_item("evals", j, R)) == "MALFORMED"
        assert tool(n, x.with_item("vs", j, R), False) == "MALFORMED"
    assert tool(n, x.but(c=R)) == "MALFORMED" and tool(n, x.but(rho=R), False) == "MALFORMED" and tool(n, x.but(pok_c=R)) == "MALFORMED"
    assert tool(n, x.but(pok_c=R), False) != "MALFORMED"             # without a DLEQ its scalars are not read
    for j in range(6):
        assert tool(n, x.with_item("s", j, R)) == "MALFORMED", j
        assert tool(n, x.with_item("s", j, R - 1)) != "MALFORMED", j


# ---- errors that need no device ---------------------------------------------------------------------------------------------------
def _load(cc, data, n_bits):
    h = ctypes.c_void_p()
    b = np.frombuffer(bytes(data), np.uint8)
    rc = cc.lib().cg_range_vk_load(ctypes.byref(h), b.ctypes.data if b.size else None, b.size, n_bits, -1)
    assert rc != OK and not h.value
    return rc, cc.lib().cg_last_error()


def test_load_errors_are_reported_before_any_hip_call(cc):
    """each with its own code: a HIP call on a box without a device would have answered CG_ERR_NO_DEVICE / CG_ERR_HIP"""
    K = RV.key(4)
    good = V.vk_bytes(K)
    assert len(good) == 640 and len(V.vk_bytes(K, beta_h_inf=True)) == 640
    h = ctypes.c_void_p()
    assert cc.lib().cg_range_vk_load(None, good, len(good), 4, -1) == INVALID_ARGUMENT
    assert cc.lib().cg_range_vk_load(ctypes.byref(h), None, 0, 4, -1) == INVALID_ARGUMENT
    for n_bits in (0, 1, 3, 5, 33, 64):
        rc, msg = _load(cc, good, n_bits)
        assert rc == INVALID_ARGUMENT and b"n_bits" in msg, n_bits
    for bad in (good[:-1], good + b"\0", bytes(7)):
        rc, msg = _load(cc, bad, 4)
        assert rc == PARSE and b"640" in msg
    for at in (0, 32, 128, 128 + 96, 256 + 32, 384 + 64):           # a coordinate of g, of h, of beta_h, of com_f_basis[0] set to q
        not_canonical = bytearray(good)
        not_canonical[at:at + 32] = RV.fe(V.Q)
        assert _load(cc, not_canonical, 4)[0] == PARSE, at
    for last in (63, 127, 255, 383, 447, 639):                      # both flags set on each kind of point
        both_flags = bytearray(good)
        both_flags[last] |= 0xC0
        assert _load(cc, both_flags, 4)[0] == PARSE, last
    with pytest.raises(cc.CrescentGpuError):
        cc.RangeVerifyingKey(good[:-1], 4)


def test_calls_report_a_null_handle_before_any_hip_call(cc):
    L = cc.lib()
    buf = (ctypes.c_uint8 * 2048)()
    slot = ctypes.c_uint32()
    for n in (0, 1):
        assert L.cg_range_verify_batch(None, 0, buf, buf, buf, buf, buf, buf, buf, buf, buf, buf, buf, n, buf, buf) == INVALID_ARGUMENT
    assert b"null" in L.cg_last_error()
    assert L.cg_range_vk_add_bases(None, buf, ctypes.byref(slot)) == INVALID_ARGUMENT
    a, b = ctypes.c_float(), ctypes.c_float()
    assert L.cg_range_vk_last_kernel_ms(None, ctypes.byref(a), ctypes.byref(b)) == INVALID_ARGUMENT
    L.cg_range_vk_free(None)


def test_compressing_a_commitment_is_a_flag_bit():
    from crescent_credentials_amd import api
    rng = random.Random(34)
    for _ in range(8):
        P = RV.g1(rng.randrange(R))
        assert api._g1_compress(V.unc(P)).tobytes() == V.o.g1_compressed(P)
    assert api._g1_compress(V.unc(None)).tobytes() == V.o.g1_compressed(None)


def test_entries_are_declared_exported_and_bound(cc):
    from crescent_credentials_amd import api
    hdr = open(os.path.join(ROOT, "include", "crescent_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "sys.rs")).read()
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "lib.rs")).read()
    L = ctypes.CDLL(cc.library_path())
    for name, n_args in (("cg_range_vk_load", 5), ("cg_range_vk_add_bases", 3), ("cg_range_vk_last_kernel_ms", 3), ("cg_range_verify_batch", 16)):
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert hasattr(L, name) and len(api._SIGNATURES[name][1]) == n_args
        assert re.search(r"pub fn %s\s*\(" % name, sys_rs), name
        assert "sys::%s" % name in lib_rs, name
    assert hasattr(L, "cg_range_vk_free") and "sys::cg_range_vk_free" in lib_rs
    assert code.index("cg_range_respond_batch") < code.index("cg_range_vk_load")             # after the creation entries
    for f in (cc.Groth16.range_verify_batch_packed, cc.Groth16.verify_range_batch, cc.RangeVerifyingKey.add_bases,
              cc.RangeVerifyingKey.last_kernel_ms, cc.RangeVerifyingKey.close):
        assert callable(f)
