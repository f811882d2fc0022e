"""Showings on the GPU (csrc/verify.hip, cg_verify_show_batch): `ShowGroth16::verify` (creds/src/groth16rand.rs:232-306)
up to the Merlin transcript, for batches of showings under one key and one io_types layout.  Every verdict is compared
with the oracle's `verify_proof_with_prepared_inputs` on the prepared inputs of groth16rand.rs:246-279, every k_out byte
with the oracle's recomputed k_i (creds/src/dlog.rs:137-145) in ark's compressed encoding (bn254_oracle.g1_compressed).
Vectors: tests/show_vectors.py."""
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
Q, R = o.Q, o.R
LAYOUTS = ["revealed", "hidden", "committed", "mixed"]


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


def _layout(name, ell):
    return {"revealed": [S.REVEALED] * ell, "hidden": [S.HIDDEN] * ell, "committed": [S.COMMITTED] * ell,
            "mixed": S.jwt_like_layout(ell)}[name]


def _pvks(cc, vk):
    return cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(vk))), ark_files.prepare_verifying_key(vk)


def _synthetic(ell, seed, ks0=None):
    """a gamma = 1 key from chosen scalars (show_groth16's C' = C - (acc_r + z) G needs gamma = 1), inputs, a proof"""
    rng = random.Random(seed)
    alpha, beta, delta = (rng.randrange(1, R) for _ in range(3))
    ks = [rng.randrange(R) for _ in range(ell + 1)]
    xs = [rng.randrange(R) for _ in range(ell)]
    if ks0 is not None:
        ks[0] = ks0(xs, ks, delta)
    sc = (alpha, beta, 1, delta, ks)
    proof = V.synthetic_proof(sc, xs, a=rng.randrange(1, R), b=rng.randrange(1, R))
    return rng, sc, V.synthetic_vk(*sc[:4], ks), xs, proof


def _golden(name):
    pk, _, w, g = V.golden_vk(name)
    rd = ark_files._Rd(bytes.fromhex(g["proofs"][0]["proof"]))
    return pk["vk"], w[1:g["num_inputs"]], (rd.g1(), rd.g2(), rd.g1())


def _expect(ora, vk, io, sh):
    return (ACCEPT if S.accepts(ora, vk, io, sh) else REJECT), S.k_bytes(S.recomputed_k(vk, io, sh))


def _run_and_compare(cc, gpu, ora, vk, io, shows):
    got_v, got_k = cc.Groth16.verify_show_batch(gpu, io, [S.api_show(cc, sh) for sh in shows])
    assert got_k.shape == (len(shows), io.count(S.COMMITTED) + 1, 32)
    out = []
    for i, sh in enumerate(shows):
        want_v, want_k = _expect(ora, vk, io, sh)
        print("showing %d: verdict %d (oracle %d), k %s (oracle %s)" % (i, got_v[i], want_v, got_k[i].tobytes().hex(), want_k.hex()))
        assert got_v[i] == want_v, i
        assert got_k[i].tobytes() == want_k, i
        out.append(want_v)
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["tiny", "d8", "dummy1024"])
def test_golden_keys(cc, name, layout):
    vk, xs, proof = _golden(name)
    io = _layout(layout, len(xs))
    gpu, ora = _pvks(cc, vk)
    with gpu:
        sh = S.make_show(vk, proof, xs, io, random.Random(len(name)))
        assert _run_and_compare(cc, gpu, ora, vk, io, [sh]) == [ACCEPT]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("ell", [1, 2, 26])
def test_synthetic_keys(cc, ell, layout):
    rng, sc, vk, xs, proof = _synthetic(ell, 300 + ell)
    io = _layout(layout, ell)
    gpu, ora = _pvks(cc, vk)
    with gpu:
        sh = S.make_show(vk, proof, xs, io, rng)
        assert _run_and_compare(cc, gpu, ora, vk, io, [sh]) == [ACCEPT]


def test_two_rerandomisations_of_one_proof(cc):
    """both accept, and no coordinate of A, B, C survives: each of the eight 32-byte field elements of the 256 proof bytes
    differs (single bytes of two unrelated field elements coincide once in 256 by chance, so whole elements are compared)"""
    rng, sc, vk, xs, proof = _synthetic(5, 77)
    io = _layout("mixed", 5)
    gpu, ora = _pvks(cc, vk)
    with gpu:
        a, b = S.make_show(vk, proof, xs, io, rng), S.make_show(vk, proof, xs, io, rng)
        assert _run_and_compare(cc, gpu, ora, vk, io, [a, b]) == [ACCEPT, ACCEPT]
    pa, pb, p0 = (o.proof_uncompressed(p) for p in (a.rand_proof, b.rand_proof, proof))
    for at in range(0, 256, 32):
        assert len({pa[at:at + 32], pb[at:at + 32], p0[at:at + 32]}) == 3


def test_tampered_slots(cc):
    """one tampered showing per odd slot, an untouched one on every even slot.

    Swapping two committed points cannot change the Groth16 verdict: they enter the prepared inputs only through their sum
    (groth16rand.rs:269), so the oracle's `verify_proof_with_prepared_inputs` accepts and so must the GPU.  What rejects
    such a showing in `ShowGroth16::verify` is the DLogPoK: both recomputed k_i change, so the challenge the host derives
    from k_out no longer equals c.  The case therefore asserts the oracle's verdict (ACCEPT) and that both k_i differ from
    the ones the prover hashed; every other tampered slot is REJECT or MALFORMED by the verdict itself."""
    rng, sc, vk, xs, proof = _synthetic(6, 91)
    io = _layout("mixed", 6)
    n_stmt = io.count(S.COMMITTED) + 1
    good = S.make_show(vk, proof, xs, io, rng)
    other = S.make_show(vk, proof, xs, io, rng)
    gpu, ora = _pvks(cc, vk)
    zero_k = bytes(32 * n_stmt)

    def clone(**kw):
        d = dict(rand_proof=good.rand_proof, com_hidden=good.com_hidden, committed=list(good.committed), c=good.c,
                 s=[list(si) for si in good.s], revealed=list(good.revealed))
        d.update(kw)
        return S.Show(**d)

    cases = []          # (what, (ShowGroth16, revealed), verdict, k bytes)

    def oracle_case(what, sh, verdict):
        v, k = _expect(ora, vk, io, sh)
        assert v == verdict, what
        cases.append((what, S.api_show(cc, sh), v, k))

    rev = list(good.revealed); rev[0] = (rev[0] + 1) % R
    oracle_case("a flipped revealed input", clone(revealed=rev), REJECT)
    swapped = clone(committed=good.committed[::-1])
    oracle_case("two committed points swapped", swapped, ACCEPT)
    k_swapped = S.recomputed_k(vk, io, swapped)
    assert k_swapped[0] != good.k[0] and k_swapped[1] != good.k[1] and k_swapped[2] == good.k[2]
    oracle_case("com_hidden replaced by another valid point", clone(com_hidden=other.com_hidden), REJECT)
    oracle_case("the original un-randomised C", clone(rand_proof=(good.rand_proof[0], good.rand_proof[1], proof[2])), REJECT)
    ch = good.com_hidden
    sg, x = S.api_show(cc, clone(com_hidden=(ch[0], (ch[1] + 1) % Q)))
    cases.append(("an off-curve com_hidden", (sg, x), MALFORMED, zero_k))
    sg, x = S.api_show(cc, clone())
    pt = bytearray(sg.commited_inputs[1]); pt[63] |= 0xC0
    sg.commited_inputs[1] = bytes(pt)
    cases.append(("a committed point with flags 0xC0", (sg, x), MALFORMED, zero_k))
    s = [list(si) for si in good.s]; s[-1][0] = R
    cases.append(("a response equal to r", S.api_show(cc, clone(s=s)), MALFORMED, zero_k))
    cases.append(("c = r + 1", S.api_show(cc, clone(c=R + 1)), MALFORMED, zero_k))
    good_v, good_k = _expect(ora, vk, io, good)
    assert good_v == ACCEPT
    batch, want_v, want_k = [], [], []
    for what, show, v, k in cases:
        batch += [S.api_show(cc, good), show]
        want_v += [ACCEPT, v]
        want_k += [good_k, k]
    with gpu:
        got_v, got_k = cc.Groth16.verify_show_batch(gpu, io, batch)
    labels = [w for c in cases for w in ("untouched", c[0])]
    for i, what in enumerate(labels):
        print("%-45s verdict %d (want %d)  k %s" % (what, got_v[i], want_v[i], got_k[i].tobytes().hex()))
    assert list(got_v) == want_v, [(w, g) for w, g in zip(labels, got_v)]
    for i, what in enumerate(labels):
        assert got_k[i].tobytes() == want_k[i], what


def test_identity_cases(cc):
    ell = 5
    io = _layout("mixed", ell)
    rs, z = [11 ** 40 % R, 13 ** 40 % R], 17 ** 40 % R
    # prepared inputs = O: k_0 cancels sum x_i k_i + (acc_r + z) delta
    cancel = lambda xs, ks, delta: (-(sum(x * k for x, k in zip(xs, ks[1:])) + (sum(rs) + z) * delta)) % R
    rng, sc, vk, xs, proof = _synthetic(ell, 501, ks0=cancel)
    sh = S.make_show(vk, proof, xs, io, rng, rs=rs, z=z)
    assert S.prepared_inputs(vk, io, sh) is None
    gpu, ora = _pvks(cc, vk)
    with gpu:
        assert _run_and_compare(cc, gpu, ora, vk, io, [sh]) == [ACCEPT]
    # a k_i = O: nonces (t, -t k / delta) on the bases (k G, delta G) of the first committed input
    rng, sc, vk, xs, proof = _synthetic(ell, 502)
    delta, ks = sc[3], sc[4]
    t = rng.randrange(1, R)
    first = io.index(S.COMMITTED)
    sh = S.make_show(vk, proof, xs, io, rng, rho={0: [t, (-t * ks[first + 1] * pow(delta, R - 2, R)) % R]})
    assert sh.k[0] is None and sh.k[1] is not None
    gpu, ora = _pvks(cc, vk)
    with gpu:
        got_v, got_k = cc.Groth16.verify_show_batch(gpu, io, [S.api_show(cc, sh)])
        assert list(got_v) == [ACCEPT]
        assert got_k[0, 0].tobytes() == bytes(31) + b"\x40"
        assert _run_and_compare(cc, gpu, ora, vk, io, [sh]) == [ACCEPT]
        # com_hidden = O: no hidden inputs and z = 0
        io_r = _layout("revealed", ell)
        sh = S.make_show(vk, proof, xs, io_r, rng, z=0)
        assert sh.com_hidden is None
        assert _run_and_compare(cc, gpu, ora, vk, io_r, [sh]) == [ACCEPT]
        # and a statement whose y is O with c != 0: the variable-base lane adds nothing
        assert sh.c != 0


def _pack(shows):
    """flat arrays of cg_verify_show_batch for a list of show_vectors.Show (all of one layout), one row per showing"""
    rows = lambda parts: np.stack([np.frombuffer(p, np.uint8) for p in parts])
    fe = lambda xs: b"".join(int(x).to_bytes(32, "little") for x in xs)
    return dict(revealed=rows([fe(sh.revealed) for sh in shows]), rand_proofs=rows([o.proof_uncompressed(sh.rand_proof) for sh in shows]),
                com_hidden=rows([o.g1_uncompressed(sh.com_hidden) for sh in shows]),
                committed=rows([b"".join(o.g1_uncompressed(P) for P in sh.committed) for sh in shows]),
                pok_c=rows([fe([sh.c]) for sh in shows]), pok_s=rows([fe([x for si in sh.s for x in si]) for sh in shows]))


@pytest.fixture(scope="module")
def cycle():
    """a short cycle of accepting and rejecting showings (length 3: never in step with the 64-lane blocks)"""
    rng, sc, vk, xs, proof = _synthetic(4, 640)
    io = _layout("mixed", 4)
    a = S.make_show(vk, proof, xs, io, rng)
    b = S.make_show(vk, proof, xs, io, rng)
    rev = list(a.revealed); rev[-1] = (rev[-1] + 1) % R
    bad = S.Show(b.rand_proof, b.com_hidden, b.committed, b.c, b.s, rev)
    ora = ark_files.prepare_verifying_key(vk)
    shows = [a, bad, b]
    want = [_expect(ora, vk, io, sh) for sh in shows]
    assert [w[0] for w in want] == [ACCEPT, REJECT, ACCEPT]
    return vk, io, _pack(shows), np.array([w[0] for w in want], np.uint8), np.stack([np.frombuffer(w[1], np.uint8) for w in want])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 32769])
def test_batch_sizes(cc, cycle, n):
    vk, io, packed, want_v, want_k = cycle
    sel = np.arange(n) % 3
    args = {k: np.ascontiguousarray(v[sel]).reshape(-1) for k, v in packed.items()}
    with cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(vk))) as gpu:
        got_v, got_k = cc.Groth16.verify_show_batch_packed(gpu, io, **args)
        assert got_v.shape == (n,) and got_k.shape == (n, io.count(S.COMMITTED) + 1, 32)
        assert np.array_equal(got_v, want_v[sel]), np.nonzero(got_v != want_v[sel])[0][:10]
        assert np.array_equal(got_k.reshape(n, -1), want_k[sel]), np.nonzero((got_k.reshape(n, -1) != want_k[sel]).any(axis=1))[0][:10]
        # pok_c = NULL: the Groth16 half only, the same verdicts, no k_out
        if n in (1, 65):
            args["pok_c"] = args["pok_s"] = None
            v2, k2 = cc.Groth16.verify_show_batch_packed(gpu, io, **args)
            assert k2 is None and np.array_equal(v2, got_v)


def test_argument_errors(cc, cycle):
    vk, io, packed, _, _ = cycle
    L = cc.lib()
    buf = {k: np.ascontiguousarray(v[:1]).reshape(-1) for k, v in packed.items()}
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    verdict = np.zeros(1, np.uint8)
    k_out = np.zeros(32 * (io.count(S.COMMITTED) + 1), np.uint8)
    with cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(vk))) as gpu:
        def call(io_bytes, n=1):
            arr = np.array(io_bytes, np.uint8)
            return L.cg_verify_show_batch(gpu._h, p(arr), arr.size, p(buf["revealed"]), p(buf["rand_proofs"]), p(buf["com_hidden"]),
                                          p(buf["committed"]), p(buf["pok_c"]), p(buf["pok_s"]), n, p(verdict), p(k_out))
        assert call(io + [S.REVEALED]) == -6                  # CG_ERR_MALFORMED_KEY
        assert call(io[:-1]) == -6
        assert call(io[:-1] + [3]) == -1                      # CG_ERR_INVALID_ARGUMENT
        assert call(io, n=0) == 0
        assert call(io) == 0 and verdict[0] == ACCEPT


def test_plain_verifier_is_unchanged(cc):
    """an all-revealed layout with com_hidden = O is `verify_with_processed_vk`: the verdicts of cg_verify_batch on the same
    inputs and the same (re-randomised) proofs"""
    rng, sc, vk, xs, proof = _synthetic(3, 808)
    io = _layout("revealed", 3)
    a = S.make_show(vk, proof, xs, io, rng, z=0)
    flipped = list(xs); flipped[1] = (flipped[1] + 1) % R
    b = S.Show(a.rand_proof, None, [], a.c, a.s, flipped)
    off = (a.rand_proof[0][0], (a.rand_proof[0][1] + 1) % Q)
    c = S.Show((off, a.rand_proof[1], a.rand_proof[2]), None, [], a.c, a.s, list(xs))
    shows = [a, b, c, a]
    with cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(vk))) as gpu:
        got_v, _ = cc.Groth16.verify_show_batch(gpu, io, [S.api_show(cc, sh) for sh in shows])
        plain = cc.Groth16.verify_batch(gpu, [sh.revealed for sh in shows], [o.proof_uncompressed(sh.rand_proof) for sh in shows])
    assert list(plain) == [ACCEPT, REJECT, MALFORMED, ACCEPT]
    assert list(got_v) == list(plain)
