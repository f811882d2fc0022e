"""Values through the GPU verifier (csrc/verify.hip: cg_verify_batch, cg_verify_show_batch, over pairing.hpp and
curve.hpp), bit-exact against what follows from arithmetic mod r and against the oracle: a thousand distinct proofs through
the device pairing, scalars that steer the 8-bit fixed-base digit walk (zero bytes, digit 255, the top window, r - 1), the
top bits of the c·y double-and-add, and partial sums that coincide or cancel in the middle of the chains of k_vfy_check,
k_show_check and k_show_k with the chain going on afterwards.  tests/test_verify_values_cpu.py shows, without a GPU, that
each crafted vector is what it claims.  Vectors: tests/verify_vectors.py, tests/show_vectors.py.  Every test gathers all
of its mismatches before it fails, so one run names every case that is wrong."""
import time

import numpy as np
import pytest

import ark_files
import bn254_oracle as o
import show_vectors as S
import verify_vectors as V

pytestmark = pytest.mark.gpu

REJECT, ACCEPT, MALFORMED = 0, 1, 2
R = o.R


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


def _vk(sc):
    return V.synthetic_vk(*sc[:4], sc[4])


def _pvk(cc, vk):
    return cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(vk)))


def _verdicts(cc, pvk, inputs, proofs):
    ib = np.frombuffer(b"".join(V.inputs_bytes(x) for x in inputs), np.uint8)
    return list(cc.Groth16.verify_batch(pvk, ib, np.frombuffer(b"".join(V.proof_bytes(p) for p in proofs), np.uint8)))


def _wrong(got, want, labels=None):
    """(slot or label, got, want) of every mismatch"""
    assert len(got) == len(want)
    return [(labels[i] if labels else i, int(g), int(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]


ORACLE_SLOTS = [0, 1, 62, 63, 64, 65, 998, 999]       # both parities on either side of the first block edge and at the end


def test_distinct_proofs(cc):
    """n = 1000 distinct proofs under one key with ell = 3 (one chunk, no multiple of the 64-lane block): all ACCEPT; then
    every odd slot tampered in one of four rotating ways: ACCEPT on the even slots, REJECT on the odd ones.  The expected
    verdicts come from the construction (the builder asserts ab = alpha beta + K gamma + c delta, or its failure, per slot);
    eight slots of each batch are confirmed by the oracle.  The same batches through cg_verify_show_batch in an all-revealed
    layout (com_hidden = O, pok_c = NULL) give the same verdicts."""
    n = 1000
    t0 = time.perf_counter()
    rng, sc = V.synthetic_scalars(3, 1000)
    vk = _vk(sc)
    inputs, scalars, proofs = V.distinct_proofs(sc, n, rng, cc)
    t_in, t_pr, how = V.interleave_tampered(sc, inputs, scalars, proofs)
    assert {h for h in how[1::2]} == set(V.TAMPERINGS) and not any(how[0::2])
    want_t = [ACCEPT if h is None else REJECT for h in how]
    t1 = time.perf_counter()
    io = [S.REVEALED] * 3
    no_hidden = np.frombuffer(o.g1_uncompressed(None) * n, np.uint8)
    wrong = {}
    with _pvk(cc, vk) as pvk:
        for what, xs, prs, want in (("distinct", inputs, proofs, [ACCEPT] * n), ("tampered", t_in, t_pr, want_t)):
            wrong[what + ", cg_verify_batch"] = _wrong(_verdicts(cc, pvk, xs, prs), want)
            got, k = cc.Groth16.verify_show_batch_packed(
                pvk, io, np.frombuffer(b"".join(V.inputs_bytes(x) for x in xs), np.uint8),
                np.frombuffer(b"".join(V.proof_bytes(p) for p in prs), np.uint8), no_hidden, np.zeros(0, np.uint8))
            assert k is None
            wrong[what + ", cg_verify_show_batch"] = _wrong(got, want)
    t2 = time.perf_counter()
    ora = ark_files.prepare_verifying_key(vk)
    for i in ORACLE_SLOTS:
        assert ark_files.verify_with_processed_vk(ora, inputs[i], proofs[i]), i
        assert ark_files.verify_with_processed_vk(ora, t_in[i], t_pr[i]) == (want_t[i] == ACCEPT), (i, how[i])
    print("building the vectors %.2f s, four GPU batches of %d %.2f s, the oracle on %d slots %.2f s"
          % (t1 - t0, n, t2 - t1, 2 * len(ORACLE_SLOTS), time.perf_counter() - t2))
    for what, w in wrong.items():
        print("%s: %d wrong verdicts (slot, got, want) %s" % (what, len(w), w[:12]))
    assert not any(wrong.values()), {k: (len(w), w[:12]) for k, w in wrong.items() if w}


def test_digit_patterns_plain_verifier(cc):
    """ell = 12: in proof p the input at position j is DIGIT_PATTERNS[(j + p) mod 12], so every fixed-base table meets every
    pattern and r - 1 occurs as a valid input.  All ACCEPT; one input of each proof bumped: all REJECT."""
    rng, sc = V.synthetic_scalars(12, 23)
    vk = _vk(sc)
    inputs, proofs, bumped = V.digit_pattern_proofs(sc, rng, cc)
    with _pvk(cc, vk) as pvk:
        got = _verdicts(cc, pvk, inputs + bumped, proofs + proofs)
    ora = ark_files.prepare_verifying_key(vk)
    for p in (0, 7):
        assert ark_files.verify_with_processed_vk(ora, inputs[p], proofs[p])
        assert not ark_files.verify_with_processed_vk(ora, bumped[p], proofs[p])
    labels = ["proof %d" % p for p in range(12)] + ["proof %d, one input bumped" % p for p in range(12)]
    wrong = _wrong(got, [ACCEPT] * 12 + [REJECT] * 12, labels)
    assert not wrong, wrong


def test_coincident_partial_sums_plain_verifier(cc):
    """k_vfy_check's chain gamma_abc[0] + sum x_i gamma_abc[i]: a doubling against the affine-lifted g0, O mid-chain with a
    restart, a doubling with zz != 1 on both sides, a cancellation before a last non-zero input, prepared inputs = O in the
    last step; and a key with g0 = O, an O entry under a non-zero input and two equal entries under equal inputs.  Each case
    is one accepting proof and the same proof with another C; every verdict is the oracle's."""
    wrong = []
    keys = {}
    for name, sc, xs, events, pi_is_o, good, bad in V.coincident_input_cases():
        if id(sc) not in keys:
            vk = _vk(sc)
            keys[id(sc)] = (_pvk(cc, vk), ark_files.prepare_verifying_key(vk))
        gpu, ora = keys[id(sc)]
        want = [ACCEPT if ark_files.verify_with_processed_vk(ora, xs, pr) else REJECT for pr in (good, bad)]
        assert want == [ACCEPT, REJECT], name
        got = _verdicts(cc, gpu, [xs, xs], [good, bad])
        print("%-100s %s (oracle %s)" % (name, [int(g) for g in got], want))
        wrong += _wrong(got, want, [name, name + " / another C"])
    for gpu, _ in keys.values():
        gpu.close()
    assert not wrong, wrong


def _show_results(cc, gpu, io, shows):
    got_v, got_k = cc.Groth16.verify_show_batch(gpu, io, [S.api_show(cc, sh) for sh in shows])
    assert got_k.shape == (len(shows), io.count(S.COMMITTED) + 1, 32)
    return [int(v) for v in got_v], [got_k[i].tobytes() for i in range(len(shows))]


def test_showings_c_and_response_values(cc):
    """one accepting showing (`mixed`, ell = 6) with c overwritten by 0, 1, 2^248 - 1, 2^253, r - 1 and the responses by
    the digit patterns.  No valid proofs of knowledge, and they need not be: the verdict depends on neither, so it stays
    ACCEPT, and every k_out byte is what dlog.rs:137-145 recomputes for the showing as it stands."""
    vk, io, base = S.pattern_show_base()
    shows = S.pattern_showings(base, V.DIGIT_PATTERNS)
    ora = ark_files.prepare_verifying_key(vk)
    assert S.accepts(ora, vk, io, base)
    pi = S.prepared_inputs(vk, io, base)
    assert all(sh.rand_proof == base.rand_proof and S.prepared_inputs(vk, io, sh) == pi for sh in shows)   # so: one verdict
    want_k = [S.k_bytes(S.recomputed_k(vk, io, sh)) for sh in shows]
    with _pvk(cc, vk) as gpu:
        got_v, got_k = _show_results(cc, gpu, io, shows)
    labels = ["c = %#x" % sh.c for sh in shows]
    wrong = _wrong(got_v, [ACCEPT] * len(shows), labels)
    for i, sh in enumerate(shows):
        for j in range(len(want_k[i]) // 32):
            g, w = got_k[i][32 * j:32 * j + 32], want_k[i][32 * j:32 * j + 32]
            if g != w:
                wrong.append(("showing %d, %s, k_%d" % (i, labels[i], j), g.hex(), w.hex()))
    flags = {kb[32 * j + 31] & 0xC0 for kb in got_k for j in range(len(kb) // 32)}
    assert not wrong, wrong
    assert flags == {0x00, 0x80}                      # a k with y of either sign


def test_showings_coincident_partial_sums(cc):
    """honest showings whose chains coincide: in k_show_check com_hidden = g0 (madd's dbl_affine), com_hidden = -g0 (O, a
    committed point restarts), committed[0] = g0 + com_hidden, a revealed partial equal to the running sum; in k_show_k,
    for a committed and for the hidden statement, s_0 base_0 = c y, s_0 base_0 = -c y with s_1 base_1 != O, and for the
    hidden statement a coincidence at the second add.  Each stands between two ordinary showings, whose results must be
    what they are on their own; verdicts and all k bytes are the oracle's."""
    vk, io, ordinary, cases = S.coincident_show_cases()
    ora = ark_files.prepare_verifying_key(vk)
    expect = lambda sh: (ACCEPT if S.accepts(ora, vk, io, sh) else REJECT, S.k_bytes(S.recomputed_k(vk, io, sh)))
    batch, labels = [ordinary[0]], ["ordinary 0"]
    for i, (name, sh, _, _, _) in enumerate(cases):
        batch += [sh, ordinary[(i + 1) % 2]]
        labels += [name, "ordinary %d after: %s" % ((i + 1) % 2, name)]
    want_ord = [expect(sh) for sh in ordinary]
    want = [want_ord[0]]
    for i, (name, sh, _, _, _) in enumerate(cases):
        want += [expect(sh), want_ord[(i + 1) % 2]]
    assert all(v == ACCEPT for v, _ in want)
    with _pvk(cc, vk) as gpu:
        got_v, got_k = _show_results(cc, gpu, io, batch)
        alone_v, alone_k = _show_results(cc, gpu, io, ordinary)
    assert list(zip(alone_v, alone_k)) == want_ord
    wrong = _wrong(got_v, [v for v, _ in want], labels)
    wrong += [(labels[i], got_k[i].hex(), want[i][1].hex()) for i in range(len(batch)) if got_k[i] != want[i][1]]
    for w in wrong:
        print(w)
    assert not wrong, wrong
