"""Creating showings on the GPU (csrc/verify.hip, cg_show_commit_batch + the host-only cg_show_respond_batch):
`ClientState::show_groth16` (creds/src/groth16rand.rs:100-187) up to the Merlin transcript, for batches of client states
under one key and one io_types layout.  Every output byte is compared with `show_vectors.make_show` given the same random
values: the re-randomised proof, com_hidden, the committed points (ark-serialize uncompressed), the k_i (compressed) and
the responses.  Vectors: tests/show_create_vectors.py."""
import ctypes
import random

import numpy as np
import pytest

import ark_files
import bn254_oracle as o
import show_create_vectors as M
import show_vectors as S
import verify_vectors as V

pytestmark = pytest.mark.gpu

ACCEPT = 1
R, Q = o.R, o.Q


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


def _gpu_key(cc, vk):
    return cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(vk)))


def _commit(cc, gpu, io, made):
    proofs, inputs, rand = M.pack(made)
    return cc.Groth16.show_commit_batch_packed(gpu, io, proofs.reshape(-1), inputs.reshape(-1), rand.reshape(-1))


def _compare(io, made, got, names=None):
    """every output row of a commit call against the oracle's bytes"""
    rp, comh, comm, k, status = got
    for i, m in enumerate(made):
        what = names[i] if names else i
        w_rp, w_comh, w_comm, w_k, _ = M.expected(io, m)
        print("%s: status %d\n  rand_proof %s\n  com_hidden %s\n  k %s" % (what, status[i], rp[i].tobytes().hex(), comh[i].tobytes().hex(),
                                                                            k[i].tobytes().hex()))
        assert status[i] == (M.MADE if m.show is not None else M.MALFORMED), what
        assert rp[i].tobytes() == w_rp, what
        assert comh[i].tobytes() == w_comh, what
        assert comm[i].tobytes() == w_comm, what
        assert k[i].tobytes() == w_k, what


def _round_trip(cc, gpu, io, made, got, names=None):
    """respond with each showing's own c, assemble ShowGroth16 and verify: ACCEPT, and the verifier recomputes the same k"""
    rp, comh, comm, k, status = got
    _, inputs, rand = M.pack(made)
    n_com, n_hid, n_resp, _ = M.counts(io)
    cs = [m.show.c for m in made]
    s = cc.Groth16.show_respond_batch(io, inputs, rand, cs, status)
    shows = []
    for i, m in enumerate(made):
        assert s[i].tobytes() == M.expected(io, m)[4], names[i] if names else i
        flat = [int.from_bytes(s[i, j].tobytes(), "little") for j in range(n_resp)]
        pok_s = [flat[2 * j:2 * j + 2] for j in range(n_com)] + [flat[2 * n_com:]]
        sg = cc.ShowGroth16(rp[i].tobytes(), comh[i].tobytes(), cs[i], pok_s, [comm[i, j].tobytes() for j in range(n_com)])
        shows.append((sg, [x for x, t in zip(m.inputs, io) if t == S.REVEALED]))
    verdicts, k_verify = cc.Groth16.verify_show_batch(gpu, io, shows)
    assert list(verdicts) == [ACCEPT] * len(made), [(names[i] if names else i) for i, v in enumerate(verdicts) if v != ACCEPT]
    assert np.array_equal(k_verify, k)


def _golden(name):
    pk, _, w, g = V.golden_vk(name)
    rd = ark_files._Rd(bytes.fromhex(g["proofs"][0]["proof"]))
    return pk["vk"], w[1:g["num_inputs"]], (rd.g1(), rd.g2(), rd.g1())


@pytest.mark.parametrize("layout", M.LAYOUTS)
@pytest.mark.parametrize("name", ["tiny", "d8"])
def test_golden_keys(cc, name, layout):
    vk, xs, proof = _golden(name)
    io = M.layout(layout, len(xs))
    m = M.make(vk, proof, xs, io, random.Random(len(name) + len(layout)))
    with _gpu_key(cc, vk) as gpu:
        _compare(io, [m], _commit(cc, gpu, io, [m]))


@pytest.mark.parametrize("layout", M.LAYOUTS)
@pytest.mark.parametrize("ell", [1, 2, 6])
def test_synthetic_keys(cc, ell, layout):
    rng, sc, vk, xs, abc = M.synthetic(ell, 900 + ell)
    io = M.layout(layout, ell)
    m = M.make(vk, M.proof_of(abc), xs, io, rng)
    with _gpu_key(cc, vk) as gpu:
        _compare(io, [m], _commit(cc, gpu, io, [m]))


def test_round_trip_through_the_verifier(cc):
    rng, sc, vk, xs, abc = M.synthetic(6, 0x707)
    io = M.layout("mixed", 6)
    made = [M.make(vk, M.proof_of(abc), xs, io, rng, c=rng.randrange(1 << 248)) for _ in range(2)]
    with _gpu_key(cc, vk) as gpu:
        got = _commit(cc, gpu, io, made)
        _compare(io, made, got)
        _round_trip(cc, gpu, io, made, got)
        # the same through show_batch, the caller's transcript standing in as a function of what it is shown
        seen = []

        def challenge(i, k_bytes, committed, com_hidden):
            seen.append((i, k_bytes.tobytes(), committed.tobytes(), com_hidden.tobytes()))
            return made[i].show.c

        states = [(m.proof_bytes, m.inputs) for m in made]
        out = cc.Groth16.show_batch(gpu, io, states, challenge, rand=[m.rand for m in made])
        # and with the randomness drawn inside: other showings of the same states, which the verifier accepts with the k_i
        # the transcript was shown
        shown = []
        c = rng.randrange(1 << 248)
        drawn = cc.Groth16.show_batch(gpu, io, states, lambda i, k, *_: shown.append(k.copy()) or c)
        revealed = [x for x, t in zip(xs, io) if t == S.REVEALED]
        verdicts, k_verify = cc.Groth16.verify_show_batch(gpu, io, [(sg, revealed) for sg in drawn])
        assert list(verdicts) == [ACCEPT, ACCEPT] and np.array_equal(k_verify, np.stack(shown))
        assert len({sg.rand_proof for sg in drawn + out}) == 4
    for i, (m, sg) in enumerate(zip(made, out)):
        w_rp, w_comh, w_comm, w_k, _ = M.expected(io, m)
        assert seen[i] == (i, w_k, w_comm, w_comh)
        assert sg == S.api_show(cc, m.show)[0]
        assert sg.to_ark_bytes() == S.ark_bytes(m.show)


def test_edge_chains(cc):
    """partial sums that are O, operands that coincide or cancel, identity components of the proof, boundary values of r1 and
    windows of 0xFF (show_create_vectors.edge_cases; tests/test_show_create_cpu.py checks the vectors themselves)"""
    vk, io, cases = M.edge_cases()
    names = [c[0] for c in cases]
    made = [c[1] for c in cases]
    with _gpu_key(cc, vk) as gpu:
        got = _commit(cc, gpu, io, made)
        _compare(io, made, got, names)
        _round_trip(cc, gpu, io, made, got, names)
    k = got[3]
    i = [n.startswith("nonces (t,") for n in names].index(True)
    assert k[i, 0].tobytes() == bytes(31) + b"\x40"


@pytest.fixture(scope="module")
def cycle():
    """three client states, the middle one malformed (r2 = 0): never in step with the 64-lane blocks"""
    rng, sc, vk, xs, abc = M.synthetic(4, 0xC7C1)
    io = M.layout("mixed", 4)
    proof = M.proof_of(abc)
    a, b = M.make(vk, proof, xs, io, rng), M.make(vk, proof, xs, io, rng)
    row = list(a.rand)
    row[1] = 0
    bad = M.Made(proof, list(xs), row, None)
    made = [a, bad, b]
    want = [M.expected(io, m) for m in made]
    want = [np.stack([np.frombuffer(w[j], np.uint8) for w in want]) for j in range(4)]
    return vk, io, M.pack(made), want, np.array([M.MADE, M.MALFORMED, M.MADE], np.uint8)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 32769])
def test_batch_sizes(cc, cycle, n):
    vk, io, packed, want, want_status = cycle
    sel = np.arange(n) % 3
    proofs, inputs, rand = (np.ascontiguousarray(a[sel]).reshape(-1) for a in packed)
    with _gpu_key(cc, vk) as gpu:
        got = cc.Groth16.show_commit_batch_packed(gpu, io, proofs, inputs, rand)
    assert np.array_equal(got[4], want_status[sel]), np.nonzero(got[4] != want_status[sel])[0][:10]
    for g, w, what in zip(got[:4], want, ("rand_proofs", "com_hidden", "committed", "k")):
        g = g.reshape(n, -1)
        assert np.array_equal(g, w[sel]), (what, np.nonzero((g != w[sel]).any(axis=1))[0][:10])


def test_malformed_slots(cc):
    rng, sc, vk, xs, abc = M.synthetic(6, 0xBAD5)
    io = M.layout("mixed", 6)
    proof = M.proof_of(abc)
    good = M.make(vk, proof, xs, io, rng)
    n_com = M.counts(io)[0]

    def variant(inputs=None, rand=None, proof_bytes=None, show=None):
        return M.Made(proof, list(good.inputs if inputs is None else inputs), list(good.rand if rand is None else rand), show,
                      good.proof_bytes if proof_bytes is None else proof_bytes)

    def with_at(seq, at, v):
        seq = list(seq)
        seq[at] = v
        return seq

    A, B, C = proof
    flagged = bytearray(good.proof_bytes)
    flagged[255] |= 0xC0
    cases = [
        ("an input >= r at a hidden position", variant(inputs=with_at(xs, io.index(S.HIDDEN), R))),
        ("a nonce = r", variant(rand=with_at(good.rand, 3 + n_com + 1, R))),
        ("r1 = 0", variant(rand=with_at(good.rand, 0, 0))),
        ("A off the curve", variant(proof_bytes=o.proof_uncompressed(((A[0], (A[1] + 1) % Q), B, C)))),
        ("flags 0xC0 on C", variant(proof_bytes=bytes(flagged))),
        ("B off the twist", variant(proof_bytes=o.proof_uncompressed((A, (B[0], ((B[1][0] + 1) % Q, B[1][1])), C)))),
        # not read, so the showing is made, and made as if the input were in range
        ("a value >= r at a revealed position", variant(inputs=with_at(xs, io.index(S.REVEALED), R + 5), show=good.show)),
    ]
    made, names = [], []
    for what, m in cases:
        made += [good, m]
        names += ["untouched", what]
    made.append(good)
    names.append("untouched")
    with _gpu_key(cc, vk) as gpu:
        got = _commit(cc, gpu, io, made)
    _compare(io, made, got, names)
    assert list(got[4]) == [M.MADE, M.MALFORMED] * 6 + [M.MADE] * 3


def test_call_errors(cc, cycle):
    vk, io, packed, _, _ = cycle
    L = cc.lib()
    proofs, inputs, rand = (np.ascontiguousarray(a[:1]).reshape(-1) for a in packed)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = [np.zeros(1024, np.uint8) for _ in range(5)]

    def call(gpu, io_bytes, n=1):
        arr = np.array(io_bytes, np.uint8)
        return L.cg_show_commit_batch(gpu._h, p(arr), arr.size, p(proofs), p(inputs), p(rand), n, *[p(a) for a in out])

    with _gpu_key(cc, vk) as gpu:
        assert call(gpu, io + [S.REVEALED]) == -6                 # CG_ERR_MALFORMED_KEY
        assert call(gpu, io[:-1]) == -6
        assert call(gpu, io[:-1] + [3]) == -1                     # CG_ERR_INVALID_ARGUMENT
        assert call(gpu, io, n=0) == 0
        assert call(gpu, io) == 0 and out[4][0] == M.MADE
    # the correction of C is sound for gamma = 1 keys only
    rng, sc, vk2, xs, abc = M.synthetic(4, 0x6A22, gamma=2)
    with _gpu_key(cc, vk2) as gpu:
        assert call(gpu, io) == -6
        assert b"gamma" in L.cg_last_error()


def test_the_verifiers_are_undisturbed(cc):
    """cg_verify_batch and cg_verify_show_batch on one handle before and after a cg_show_commit_batch call that grows the
    handle's buffers: the same verdicts and the same k bytes"""
    rng, sc, vk, xs, abc = M.synthetic(6, 0x5AFE)
    io = M.layout("mixed", 6)
    proof = M.proof_of(abc)
    made = [M.make(vk, proof, xs, io, rng) for _ in range(2)]
    shows = [S.api_show(cc, m.show) for m in made]
    tampered = S.clone(made[1].show, revealed=[(made[1].show.revealed[0] + 1) % R] + made[1].show.revealed[1:])
    shows.append(S.api_show(cc, tampered))
    flipped = list(xs)
    flipped[0] = (flipped[0] + 1) % R
    plain_inputs, plain_proofs = [xs, flipped, xs], [o.proof_uncompressed(proof)] * 3
    with _gpu_key(cc, vk) as gpu:
        v0 = cc.Groth16.verify_batch(gpu, plain_inputs, plain_proofs).copy()
        s0, k0 = (a.copy() for a in cc.Groth16.verify_show_batch(gpu, io, shows))
        many = [made[i % 2] for i in range(200)]
        got = _commit(cc, gpu, io, many)
        assert (got[4] == M.MADE).all()
        v1 = cc.Groth16.verify_batch(gpu, plain_inputs, plain_proofs)
        s1, k1 = cc.Groth16.verify_show_batch(gpu, io, shows)
    assert list(v0) == [1, 0, 1] and list(s0) == [1, 1, 0]
    assert np.array_equal(v0, v1) and np.array_equal(s0, s1) and np.array_equal(k0, k1)


def test_entries_share_the_buffers_of_one_handle(cc):
    """the three entries on one handle in growing and in shrinking order, so that each in turn is the one that last grew a
    buffer the others read (proofs, scalars, com_hidden, committed, k, the term descriptor): every call returns what the same
    call returns on a handle of its own.  The sizes cross one 64-lane workgroup; every call has one tampered or malformed
    item."""
    rng, sc, vk, xs, abc = M.synthetic(6, 0x5AFE)
    io = M.layout("mixed", 6)
    proof = M.proof_of(abc)
    made = [M.make(vk, proof, xs, io, rng) for _ in range(2)]
    tampered = S.clone(made[1].show, revealed=[(made[1].show.revealed[0] + 1) % R] + made[1].show.revealed[1:])
    shows = [S.api_show(cc, made[0].show), S.api_show(cc, tampered), S.api_show(cc, made[1].show)]
    flipped = list(xs)
    flipped[0] = (flipped[0] + 1) % R
    row = list(made[0].rand)
    row[1] = 0                                                    # r2 = 0
    bad = M.Made(proof, list(xs), row, None)

    def one_bad(n, at, good, other):
        return [other if i == at else good(i) for i in range(n)]

    def verify_show(gpu):
        v, k = cc.Groth16.verify_show_batch(gpu, io, shows)
        assert list(v) == [1, 0, 1]
        return [v.copy(), k.copy()]

    def verify(n, at):
        def call(gpu):
            v = cc.Groth16.verify_batch(gpu, one_bad(n, at, lambda i: xs, flipped), [o.proof_uncompressed(proof)] * n)
            assert list(v) == one_bad(n, at, lambda i: 1, 0)
            return [v.copy()]
        return call

    def commit(n, at):
        def call(gpu):
            got = _commit(cc, gpu, io, one_bad(n, at, lambda i: made[i % 2], bad))
            assert list(got[4]) == one_bad(n, at, lambda i: M.MADE, M.MALFORMED)
            return [a.copy() for a in got]
        return call

    calls = [verify_show, verify(130, 64), commit(70, 64), verify_show, verify(2, 1), commit(1, 0)]
    with _gpu_key(cc, vk) as gpu:
        shared = [call(gpu) for call in calls]
    for i, call in enumerate(calls):
        if i == 0:                                                # the handle was fresh then
            continue
        if i == 3:                                                # the same call as the first
            alone = shared[0]
        else:
            with _gpu_key(cc, vk) as gpu:
                alone = call(gpu)
        assert len(alone) == len(shared[i])
        for a, b in zip(alone, shared[i]):
            assert np.array_equal(a, b), i
