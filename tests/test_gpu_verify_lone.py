"""The latency arrangement of the Groth16 verifiers (cg_pvk_set_latency_mode; csrc/pairing_team.hpp, k_lone_* in
csrc/verify.hip): one workgroup per proof, and [r]B = O on a second stream beside the pairing.  Every test compares three
things with each other: what the vectors expect, the wide arrangement, and the latency arrangement on the same handle.
Vectors: tests/verify_vectors.py, tests/show_vectors.py, as they are."""
import ctypes
import random

import numpy as np
import pytest

import ark_files
import bn254_oracle as o
import show_vectors as S
import verify_vectors as V

pytestmark = pytest.mark.gpu

REJECT, ACCEPT, MALFORMED = 0, 1, 2
INVALID_ARGUMENT = -1
Q, R = o.Q, o.R
CHUNK = 1 << 15                      # proofs per launch set (csrc/verify.hip, VCHUNK)


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


def _pvk(cc, vk, **kw):
    return cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(vk)), **kw)


def _vk(sc):
    return V.synthetic_vk(*sc[:4], sc[4])


def _bytes_of(inputs, proofs):
    pb = [p if isinstance(p, bytes) else V.proof_bytes(p) for p in proofs]
    return np.frombuffer(b"".join(V.inputs_bytes(x) for x in inputs), np.uint8), np.frombuffer(b"".join(pb), np.uint8)


def both(cc, pvk, inputs, proofs, want, what=""):
    """the wide arrangement, then the latency one, on the same handle: each against `want`, and so against each other"""
    ib, pb = _bytes_of(inputs, proofs)
    got = {}
    for mode in (False, True):
        pvk.set_latency(mode)
        got[mode] = list(cc.Groth16.verify_batch(pvk, ib, pb))
    pvk.set_latency(False)
    wrong = {("latency" if m else "wide"): [(i, int(g), int(w)) for i, (g, w) in enumerate(zip(v, want)) if g != w][:12] for m, v in got.items()}
    assert len(got[False]) == len(got[True]) == len(want) and not any(wrong.values()), (what, wrong)


def test_the_setters_exist(cc):
    L = cc.lib()
    for name in ("cg_pvk_set_latency_mode", "cg_pvk_last_kernel_ms", "cg_range_vk_set_latency_mode"):
        assert hasattr(L, name), name
    rng, sc = V.synthetic_scalars(1, 1)
    a, b = ctypes.c_float(-1), ctypes.c_float(-1)
    with _pvk(cc, _vk(sc)) as pvk:
        for on in (1, 0, 1, 1, 0):
            assert L.cg_pvk_set_latency_mode(pvk._h, on) == 0
        for bad in (2, -1, 256, 1 << 30):
            assert L.cg_pvk_set_latency_mode(pvk._h, bad) == INVALID_ARGUMENT, bad
            assert b"latency mode" in L.cg_last_error()
        assert L.cg_pvk_last_kernel_ms(pvk._h, ctypes.byref(a), None) == INVALID_ARGUMENT
        assert L.cg_pvk_last_kernel_ms(pvk._h, ctypes.byref(a), ctypes.byref(b)) == 0 and a.value == 0 and b.value == 0
    assert L.cg_pvk_set_latency_mode(None, 1) == INVALID_ARGUMENT
    assert L.cg_pvk_last_kernel_ms(None, ctypes.byref(a), ctypes.byref(b)) == INVALID_ARGUMENT
    with _pvk(cc, _vk(sc), latency=True) as pvk:                # the constructor's flag
        xs = [rng.randrange(R)]
        pr = V.synthetic_proof(sc, xs, a=rng.randrange(1, R), b=rng.randrange(1, R))
        assert cc.Groth16.verify_with_processed_vk(pvk, xs, V.proof_bytes(pr))
        assert not cc.Groth16.verify_with_processed_vk(pvk, [(xs[0] + 1) % R], V.proof_bytes(pr))
        group_ms, pairing_ms = pvk.last_kernel_ms()
        assert group_ms > 0 and pairing_ms > 0


@pytest.mark.parametrize("name", ["tiny", "d8"])
def test_golden_keys(cc, name):
    pk, _, w, g = V.golden_vk(name)
    xs = w[1:g["num_inputs"]]
    golden = [bytes.fromhex(c["proof"]) for c in g["proofs"]]
    flipped = list(xs)
    flipped[0] = (flipped[0] + 1) % R
    swapped = golden[0][192:256] + golden[0][64:192] + golden[0][0:64]
    with _pvk(cc, pk["vk"]) as pvk:
        both(cc, pvk, [xs] * len(golden) + [flipped, xs], golden + [golden[0], swapped], [ACCEPT] * len(golden) + [REJECT, REJECT])
        both(cc, pvk, [xs], golden[:1], [ACCEPT])


def _tamper_c(sc, inputs, scalars, proofs):
    """for a key with fewer than three inputs (interleave_tampered bumps input i mod 3): every odd slot takes the C of the
    next slot; the verdict of every slot follows from the equation in the exponent, asserted here"""
    n = len(proofs)
    out, want = [], []
    for i in range(n):
        (a, b, c), (A, B, C) = scalars[i], proofs[i]
        if i & 1:
            c, C = scalars[(i + 1) % n][2], proofs[(i + 1) % n][2]
        holds = V.equation_holds(sc, V.prepared_scalar(sc[4], inputs[i]), a, b, c)
        assert holds == (not i & 1), i
        out.append((A, B, C))
        want.append(ACCEPT if holds else REJECT)
    return out, want


@pytest.mark.parametrize("ell", [0, 1, 3, 26])
def test_synthetic_keys_distinct_and_tampered(cc, ell):
    """65 distinct accepting proofs and the same batch with every odd slot tampered, at n = 1, 2, 3 and 65"""
    rng, sc = V.synthetic_scalars(ell, 4000 + ell)
    inputs, scalars, proofs = V.distinct_proofs(sc, 65, rng, cc)
    if ell >= 3:
        t_in, t_pr, how = V.interleave_tampered(sc, inputs, scalars, proofs)
        t_want = [ACCEPT if h is None else REJECT for h in how]
    else:
        t_in = inputs
        t_pr, t_want = _tamper_c(sc, inputs, scalars, proofs)
    with _pvk(cc, _vk(sc)) as pvk:
        for n in (1, 2, 3, 65):
            both(cc, pvk, inputs[:n], proofs[:n], [ACCEPT] * n, "distinct, n = %d" % n)
            both(cc, pvk, t_in[65 - n:], t_pr[65 - n:], t_want[65 - n:], "tampered, n = %d" % n)     # the last n: slot 64 is even


def test_digit_patterns(cc):
    rng, sc = V.synthetic_scalars(12, 4023)
    inputs, proofs, bumped = V.digit_pattern_proofs(sc, rng, cc)
    xs, prs, want = inputs + bumped, proofs + proofs, [ACCEPT] * 12 + [REJECT] * 12
    with _pvk(cc, _vk(sc)) as pvk:
        for n in (1, 2, 3):
            both(cc, pvk, bumped[:n], proofs[:n], [REJECT] * n, "bumped, n = %d" % n)
        both(cc, pvk, (xs * 3)[:65], (prs * 3)[:65], (want * 3)[:65], "n = 65")


def test_identity_skips(cc):
    """one per pair: A = O, C = O, prepared inputs = O (the cases of test_gpu_verify.py::test_synthetic_keys_identity_skips),
    B = O, and a rejecting proof; each also alone, where the whole workgroup drops the pair"""
    rng, sc = V.synthetic_scalars(2, 4100)
    alpha, beta, gamma, delta, ks = sc
    xs = [rng.randrange(R) for _ in range(2)]
    sc0 = (alpha, beta, gamma, delta, [(-sum(x * k for x, k in zip(xs, ks[1:]))) % R] + ks[1:])       # prepared inputs = O for xs
    a, b = rng.randrange(1, R), rng.randrange(1, R)
    live = V.synthetic_proof(sc, xs, a=a, b=b)
    cases = [live, V.synthetic_proof(sc, xs, a=0, b=b), V.synthetic_proof(sc, xs, a=a, b=0), V.synthetic_proof(sc, xs, a=a, c=0),
             (live[0], live[1], o.G1.to_affine(o.G1.add_affine(o.G1.to_jac(live[2]), o.G1_GEN)))]
    assert cases[1][0] is None and cases[2][1] is None and cases[3][2] is None
    want = [ACCEPT] * 4 + [REJECT]
    ora = ark_files.prepare_verifying_key(_vk(sc))
    assert ark_files.verify_with_processed_vk(ora, xs, cases[1]) and not ark_files.verify_with_processed_vk(ora, xs, cases[4])
    with _pvk(cc, _vk(sc)) as pvk:
        both(cc, pvk, [xs] * 5, cases, want)
        for pr, w in zip(cases, want):
            both(cc, pvk, [xs], [pr], [w])
    pi_o = V.synthetic_proof(sc0, xs, a=a, b=b)
    with _pvk(cc, _vk(sc0)) as pvk:
        both(cc, pvk, [xs, xs, xs], [pi_o, live, pi_o], [ACCEPT, REJECT, ACCEPT])
        both(cc, pvk, [xs], [pi_o], [ACCEPT])


def _malformed(sc, xs, good, rng):
    a, b, c = good
    gb = V.proof_bytes(good)
    out = [("B on the twist outside G2", xs, V.proof_bytes((a, V.twist_point_outside_g2(rng), c)))]
    p = bytearray(gb); p[192:224] = Q.to_bytes(32, "little")
    out.append(("C.x = q", xs, bytes(p)))
    p = bytearray(gb); p[64:96] = (Q + 5).to_bytes(32, "little")
    out.append(("B.x.c0 > q", xs, bytes(p)))
    bad_in = list(xs); bad_in[-1] = R
    out.append(("input = r", bad_in, gb))
    out.append(("off-curve A", xs, V.proof_bytes(((a[0], (a[1] + 1) % Q), b, c))))
    return out


def test_malformed_slots_between_good_ones(cc):
    rng, sc = V.synthetic_scalars(2, 4200)
    xs = [rng.randrange(R) for _ in range(2)]
    good = V.synthetic_proof(sc, xs, a=rng.randrange(1, R), b=rng.randrange(1, R))
    flipped = [xs[0], (xs[1] + 1) % R]
    cases = _malformed(sc, xs, good, rng)
    inputs, proofs, want = [xs], [good], [ACCEPT]
    for i, (_, x, p) in enumerate(cases):
        inputs += [x, flipped if i & 1 else xs]
        proofs += [p, good]
        want += [MALFORMED, REJECT if i & 1 else ACCEPT]
    with _pvk(cc, _vk(sc)) as pvk:
        both(cc, pvk, inputs, proofs, want, [c[0] for c in cases])
        for what, x, p in cases:                                # and each alone: the second stream decides the first case
            both(cc, pvk, [x], [p], [MALFORMED], what)


def test_a_batch_of_one_chunk_plus_one(cc):
    rng, sc = V.synthetic_scalars(2, 4300)
    xs = [rng.randrange(R) for _ in range(2)]
    good = V.synthetic_proof(sc, xs, a=rng.randrange(1, R), b=rng.randrange(1, R))
    flipped = [xs[0], (xs[1] + 1) % R]
    mal = _malformed(sc, xs, good, rng)[0]
    kinds = [(xs, V.proof_bytes(good), ACCEPT), (flipped, V.proof_bytes(good), REJECT), (mal[1], mal[2], MALFORMED)]
    n = CHUNK + 1
    sel = np.arange(n) % 3
    sel[-1] = 1                                                 # the lone proof of the second chunk rejects
    ib = np.stack([np.frombuffer(V.inputs_bytes(k[0]), np.uint8) for k in kinds])[sel].reshape(-1)
    pb = np.stack([np.frombuffer(k[1], np.uint8) for k in kinds])[sel].reshape(-1)
    want = np.array([k[2] for k in kinds], np.uint8)[sel]
    with _pvk(cc, _vk(sc)) as pvk:
        for mode in (False, True):
            pvk.set_latency(mode)
            got = cc.Groth16.verify_batch(pvk, ib, pb)
            assert got.shape == (n,) and np.array_equal(got, want), (mode, np.nonzero(got != want)[0][:10])


def test_mode_switching_between_calls(cc):
    """on, off, on on one handle between calls of different n: the same bytes each time"""
    rng, sc = V.synthetic_scalars(3, 4400)
    inputs, scalars, proofs = V.distinct_proofs(sc, 65, rng, cc)
    t_in, t_pr, how = V.interleave_tampered(sc, inputs, scalars, proofs)
    want = [ACCEPT if h is None else REJECT for h in how]
    with _pvk(cc, _vk(sc)) as pvk:
        for mode, n in ((True, 3), (False, 65), (True, 1), (True, 65), (False, 2), (True, 2)):
            pvk.set_latency(mode)
            ib, pb = _bytes_of(t_in[:n], t_pr[:n])
            assert list(cc.Groth16.verify_batch(pvk, ib, pb)) == want[:n], (mode, n)


# ---- showings ---------------------------------------------------------------------------------------------------------
def _show_both(cc, pvk, io, packed):
    out = {}
    for mode in (False, True):
        pvk.set_latency(mode)
        out[mode] = cc.Groth16.verify_show_batch_packed(pvk, io, **packed)
    pvk.set_latency(False)
    return out


def _pack(shows):
    rows = lambda parts: np.stack([np.frombuffer(p, np.uint8) for p in parts]).reshape(-1)
    fe = lambda xs: b"".join(int(x).to_bytes(32, "little") for x in xs)
    return dict(revealed=rows([fe(sh.revealed) for sh in shows]), rand_proofs=rows([o.proof_uncompressed(sh.rand_proof) for sh in shows]),
                com_hidden=rows([o.g1_uncompressed(sh.com_hidden) for sh in shows]),
                committed=rows([b"".join(o.g1_uncompressed(P) for P in sh.committed) for sh in shows]),
                pok_c=rows([fe([sh.c]) for sh in shows]), pok_s=rows([fe([x for si in sh.s for x in si]) for sh in shows]))


def test_showings_mixed_layout(cc):
    """ell = 26, n = 3 with a tampered slot, then a slot whose B is outside G2: its verdict AND its zeroed k_out wait for the
    second stream.  Verdicts and k_out against the oracle in both modes; then the pok_c = NULL call"""
    ell = 26
    rng = random.Random(4500)
    alpha, beta, delta = (rng.randrange(1, R) for _ in range(3))
    ks = [rng.randrange(R) for _ in range(ell + 1)]
    xs = [rng.randrange(R) for _ in range(ell)]
    sc = (alpha, beta, 1, delta, ks)
    vk = V.synthetic_vk(*sc[:4], ks)
    proof = V.synthetic_proof(sc, xs, a=rng.randrange(1, R), b=rng.randrange(1, R))
    io = S.jwt_like_layout(ell)
    n_stmt = io.count(S.COMMITTED) + 1
    a, b = S.make_show(vk, proof, xs, io, rng), S.make_show(vk, proof, xs, io, rng)
    rev = list(a.revealed)
    rev[0] = (rev[0] + 1) % R
    bad = S.Show(b.rand_proof, b.com_hidden, b.committed, b.c, b.s, rev)
    outside = S.Show((a.rand_proof[0], V.twist_point_outside_g2(rng), a.rand_proof[2]), a.com_hidden, a.committed, a.c, a.s, list(a.revealed))
    ora = ark_files.prepare_verifying_key(vk)
    want_v = [ACCEPT, REJECT, ACCEPT, MALFORMED]
    want_k = [S.k_bytes(S.recomputed_k(vk, io, sh)) for sh in (a, bad, b)] + [bytes(32 * n_stmt)]
    assert S.accepts(ora, vk, io, a) and not S.accepts(ora, vk, io, bad)
    shows = [a, bad, b, outside]
    with _pvk(cc, vk) as pvk:
        for n in (3, 4, 1):
            got = _show_both(cc, pvk, io, _pack(shows[:n]))
            for mode, (v, k) in got.items():
                assert list(v) == want_v[:n], (mode, n, list(v))
                assert [k[i].tobytes() for i in range(n)] == want_k[:n], (mode, n)
        lone = _show_both(cc, pvk, io, _pack([outside]))
        for mode, (v, k) in lone.items():
            assert list(v) == [MALFORMED] and k[0].tobytes() == bytes(32 * n_stmt), mode
        args = _pack(shows)
        args["pok_c"] = args["pok_s"] = None
        for mode, (v, k) in _show_both(cc, pvk, io, args).items():
            assert k is None and list(v) == want_v, (mode, list(v))
