"""Creating range proofs without a GPU: the host-only cg_range_respond_batch against the restatement of tests/range_vectors.py,
the argument errors of cg_range_pk_load and of the three GPU calls - every one of them is reported before any HIP call,
so they carry their own codes on a box with no device - the `RangeProof` byte layout of the package against an
independent writer, and the entries declared, exported and bound.  The restatement itself is checked here too: what it
proves, its trapdoor verifier accepts, and a changed evaluation it rejects."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT
import range_vectors as RV

R = RV.R
OK, INVALID_ARGUMENT, MALFORMED_KEY, PARSE = 0, -1, -6, -7


def _rows(rng, n, bits=4):
    return [(rng.randrange(1 << bits), rng.randrange(R), [rng.randrange(R) for _ in range(18)], rng.randrange(R)) for _ in range(n)]


def _pack(rows):
    return (b"".join(RV.fe(m) + RV.fe(r) for m, r, _, _ in rows), b"".join(RV.fes(rd) for _, _, rd, _ in rows), RV.fes(c for _, _, _, c in rows))


def _want_s(m, r, rd, c):
    nonces = [rd[RV.TM], rd[RV.TR]] + rd[RV.TF] + [rd[RV.TM]]
    return RV.fes((t - c * x) % R for t, x in zip(nonces, [m, r] + rd[RV.F] + [m]))


def test_restatement_proves_what_its_verifier_accepts():
    rng = random.Random(21)
    K = RV.key(4)
    bases = [RV.g1(rng.randrange(R)), RV.g1(rng.randrange(R))]
    m, r, rd, c_dleq = _rows(rng, 1)[0]
    x = RV.prove(K, bases, m, r, rd, c_dleq, rng.randrange(R), rng.randrange(R))
    assert x.ok == (True, True, True) and x.s[5] == x.s[0]
    com_f, com_g, ts = RV.expected_commit(x)
    evals, proofs = RV.expected_open(x)
    proof = RV.ark_bytes(com_f, com_g, evals, proofs, RV.expected_quotient(x)[0], c_dleq, x.s)
    ped = RV.msm(bases, [m, r])
    assert RV.verify(K, bases, ped, proof, x.c, x.rho, ts[64:])
    for at in (128, 128 + 32 + 64 + 1, len(proof) - 32):                     # eval_g, random_v of proof_g, s_13
        bad = bytearray(proof)
        bad[at] ^= 1
        assert not RV.verify(K, bases, ped, bytes(bad), x.c, x.rho, ts[64:]), at
    assert not RV.verify(K, bases, RV.msm(bases, [m + 1, r]), proof, x.c, x.rho, ts[64:])      # another commitment


def test_respond_batch_matches_the_restatement(cc):
    rng = random.Random(22)
    rows = _rows(rng, 5)
    rows[1] = (0, 0, rows[1][2], 0)
    rows[2] = (15, R - 1, [R - 1] * 18, R - 1)
    ob, rb, cb = _pack(rows)
    s = cc.Groth16.range_respond_batch(ob, rb, cb)
    assert s.shape == (5, 6, 32)
    for i, row in enumerate(rows):
        assert s[i].tobytes() == _want_s(*row), i
        assert s[i, 5].tobytes() == s[i, 0].tobytes()                         # s_13 == s_00: eq_pos = (0, 3)


def test_respond_batch_skips_a_row_by_its_status_byte(cc):
    rng = random.Random(23)
    rows = _rows(rng, 3)
    ob, rb, cb = _pack(rows)
    # the skipped row is not read: a value >= r in it is no error
    rb = bytearray(rb)
    rb[32 * 18 + 32 * RV.TM:32 * 18 + 32 * RV.TM + 32] = RV.fe(R)
    s = cc.Groth16.range_respond_batch(ob, bytes(rb), cb, status=bytes([1, 2, 1]))
    assert s[0].tobytes() == _want_s(*rows[0]) and s[2].tobytes() == _want_s(*rows[2])
    assert s[1].tobytes() == bytes(192)


@pytest.mark.parametrize("where", ["m", "r", "f1", "t_m", "t_f2", "c_dleq"])
def test_respond_batch_names_the_showing_of_a_value_not_below_r(cc, where):
    rng = random.Random(24)
    rows = _rows(rng, 4)
    m, r, rd, c = rows[2]
    rd = list(rd)
    if where == "m": m = R
    elif where == "r": r = R + 5
    elif where == "c_dleq": c = R
    else: rd[{"f1": 4, "t_m": 6, "t_f2": 10}[where]] = R
    rows[2] = (m, r, rd, c)
    ob, rb, cb = _pack(rows)
    out = np.full((4, 6, 32), 0xAB, np.uint8)
    L = cc.lib()
    u8 = lambda b: np.frombuffer(b, np.uint8).ctypes.data
    assert L.cg_range_respond_batch(u8(ob), u8(rb), u8(cb), None, 4, out.ctypes.data) == INVALID_ARGUMENT
    assert b"showing 2" in L.cg_last_error()
    assert (out == 0xAB).all()                                                # nothing is written
    # rand values the responses do not read may be anything
    rows[2] = (rows[1][0], rows[1][1], [R if i in (0, 11, 15) else v for i, v in enumerate(rows[1][2])], rows[1][3])
    ob, rb, cb = _pack(rows)
    assert L.cg_range_respond_batch(u8(ob), u8(rb), u8(cb), None, 4, out.ctypes.data) == OK


def test_respond_batch_argument_errors(cc):
    L = cc.lib()
    buf = (ctypes.c_uint8 * 1024)()
    assert L.cg_range_respond_batch(None, None, None, None, 0, None) == OK
    for args in ((None, buf, buf), (buf, None, buf), (buf, buf, None)):
        assert L.cg_range_respond_batch(*args, None, 1, buf) == INVALID_ARGUMENT
    assert L.cg_range_respond_batch(buf, buf, buf, None, 1, None) == INVALID_ARGUMENT
    assert b"null" in L.cg_last_error()


def _load(cc, data, n_bits):
    h = ctypes.c_void_p()
    b = np.frombuffer(bytes(data), np.uint8)
    rc = cc.lib().cg_range_pk_load(ctypes.byref(h), b.ctypes.data if b.size else None, b.size, n_bits, -1)
    assert rc != OK and not h.value
    return rc, cc.lib().cg_last_error()


def test_load_errors_are_reported_before_any_hip_call(cc):
    """each with its own code: a HIP call on a box without a device would have answered CG_ERR_NO_DEVICE / CG_ERR_HIP"""
    K = RV.key(4)
    good = K.data
    assert len(good) == 8 + 12 * 64 + 8 + 4 * 64
    h = ctypes.c_void_p()
    assert cc.lib().cg_range_pk_load(None, good, len(good), 4, -1) == INVALID_ARGUMENT
    assert cc.lib().cg_range_pk_load(ctypes.byref(h), None, 0, 4, -1) == INVALID_ARGUMENT
    for n_bits in (0, 1, 3, 5, 33, 64):
        rc, msg = _load(cc, good, n_bits)
        assert rc == INVALID_ARGUMENT and b"n_bits" in msg, n_bits
    for bad in (good[:-1], good + b"\0", good[:8 + 5 * 64], bytes(7), (2 ** 40).to_bytes(8, "little") + good[8:]):
        assert _load(cc, bad, 4)[0] == PARSE
    not_canonical = bytearray(good)
    not_canonical[8:40] = RV.fe(RV.o.Q)                                       # x = q
    assert _load(cc, not_canonical, 4)[0] == PARSE
    both_flags = bytearray(good)
    both_flags[8 + 63] |= 0xC0
    assert _load(cc, both_flags, 4)[0] == PARSE
    # enough bytes, too few powers: 2n + 4 of g, 4 of gamma_g
    assert _load(cc, RV.pk_bytes(K.pg[:11], K.pgam), 4)[0] == MALFORMED_KEY
    assert _load(cc, RV.pk_bytes(K.pg, K.pgam[:3]), 4)[0] == MALFORMED_KEY
    assert _load(cc, good, 8)[0] == MALFORMED_KEY                             # a key cut for 4 bits asked for 8
    with pytest.raises(cc.CrescentGpuError):
        cc.RangeProofKey(good[:-1], 4)


def test_gpu_calls_report_a_null_handle_before_any_hip_call(cc):
    L = cc.lib()
    buf = (ctypes.c_uint8 * 2048)()
    slot = ctypes.c_uint32()
    for n in (0, 1):
        assert L.cg_range_commit_batch(None, 0, buf, buf, n, buf, buf, buf, buf) == INVALID_ARGUMENT
        assert L.cg_range_quotient_batch(None, buf, buf, buf, n, buf, buf, buf) == INVALID_ARGUMENT
        assert L.cg_range_open_batch(None, buf, buf, buf, buf, n, buf, buf, buf) == INVALID_ARGUMENT
    assert b"null" in L.cg_last_error()
    assert L.cg_range_pk_add_bases(None, buf, ctypes.byref(slot)) == INVALID_ARGUMENT
    a, b = ctypes.c_float(), ctypes.c_float()
    assert L.cg_range_pk_last_kernel_ms(None, ctypes.byref(a), ctypes.byref(b)) == INVALID_ARGUMENT
    L.cg_range_pk_free(None)


def test_range_proof_bytes_layout(cc):
    rng = random.Random(25)
    pt = lambda: RV.o.g1_uncompressed(RV.g1(rng.randrange(R)))
    com_f, com_g, com_q = pt(), pt(), pt()
    evals = [rng.randrange(R) for _ in range(3)]
    proofs = [pt() + RV.fe(rng.randrange(R)) for _ in range(3)]
    c, s = rng.randrange(R), [rng.randrange(R) for _ in range(6)]
    mine = cc.RangeProof(com_f, com_g, evals[0], proofs[0], evals[1], proofs[1], com_q, evals[2], proofs[2], c, [s[:2], s[2:]])
    want = RV.ark_bytes(com_f, com_g, RV.fes(evals), b"".join(proofs), com_q, c, s)
    assert mine.to_bytes() == want
    # com_f com_g | eval, (W, tag, v) twice | com_q | eval, (W, tag, v) | c | 2, (2, s s), (4, s s s s)
    assert len(want) == 128 + 2 * (32 + 97) + 64 + 32 + 97 + 32 + 8 + (8 + 64) + (8 + 128)
    assert want[128 + 32 + 64] == 1 and want[:64] == com_f and want[-32:] == RV.fe(s[5])
    with pytest.raises(ValueError):
        cc.RangeProof(com_f, com_g, 0, proofs[0][:95], 0, proofs[1], com_q, 0, proofs[2], c, [s[:2], s[2:]]).to_bytes()


def test_entries_are_declared_exported_and_bound(cc):
    from crescent_credentials_amd import api
    hdr = open(os.path.join(ROOT, "include", "crescent_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    sys_rs = open(os.path.join(ROOT, "integration", "rust", "crescent-gpu", "src", "sys.rs")).read()
    L = ctypes.CDLL(cc.library_path())
    for name, n_args in (("cg_range_pk_load", 5), ("cg_range_pk_add_bases", 3), ("cg_range_commit_batch", 9),
                         ("cg_range_quotient_batch", 8), ("cg_range_open_batch", 9), ("cg_range_respond_batch", 6)):
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert hasattr(L, name) and len(api._SIGNATURES[name][1]) == n_args
        assert re.search(r"pub fn %s\s*\(" % name, sys_rs), name
    assert re.search(r"CG_RANGE_N_RAND = 18, CG_RANGE_N_RESP = 6", code)
    assert (cc.CG_RANGE_N_RAND, cc.CG_RANGE_N_RESP) == (18, 6)
    assert code.index("cg_show_respond_batch") < code.index("cg_range_pk_load")          # after the showing entries
    assert "DEVIATION" in hdr and "random_v" in hdr
    for f in (cc.Groth16.range_commit_batch_packed, cc.Groth16.range_quotient_batch_packed, cc.Groth16.range_open_batch_packed,
              cc.Groth16.range_respond_batch, cc.Groth16.show_range_batch, cc.RangeProofKey.add_bases):
        assert callable(f)
