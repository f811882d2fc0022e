"""Creating range proofs on the GPU (csrc/rangeproof.hip: cg_range_commit_batch, cg_range_quotient_batch,
cg_range_open_batch, and the host-only cg_range_respond_batch): `RangeProof::prove_n_bits`
(creds/src/rangeproof.rs:114-339) up to the Merlin transcripts, for batches of Pedersen openings under one KZG key.
Every output byte of the three calls is compared with the restatement of tests/range_vectors.py given the same random
values and challenges (MSMs over the key's points); the assembled proofs pass its trapdoor restatement of
`verify_n_bits`.  All comparisons are exact."""
import ctypes
import random

import numpy as np
import pytest

import bn254_oracle as o
import range_vectors as RV
import show_create_vectors as M

pytestmark = pytest.mark.gpu

R = RV.R
INVALID_ARGUMENT = -1
CHUNK = 1 << 12                      # showings per launch set of the three calls (csrc/rangeproof.hip, RCHUNK)
B0, B1 = 0x1234567, 0x89ABCDEF123    # the Pedersen bases' scalars: B_i = b_i G
inv = RV.inv


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


def bases_of(b0=B0, b1=B1):
    return [RV.g1(b0), RV.g1(b1)]


def bases_bytes(bases):
    return b"".join(o.g1_uncompressed(P) for P in bases)


@pytest.fixture(scope="module")
def key4(cc):
    K = RV.key(4)
    with cc.RangeProofKey(K.data, 4) as gpu:
        slot = gpu.add_bases(*[o.g1_uncompressed(P) for P in bases_of()])
        yield K, gpu, slot


def draw(rng, n_bits, at=None, **kw):
    """one opening with its rand row and challenges; kw overrides m, r, c, rho or c_dleq, `at` rand entries by index"""
    d = dict(m=rng.randrange(1 << n_bits), r=rng.randrange(R), c=rng.randrange(R), rho=rng.randrange(R), c_dleq=rng.randrange(R))
    rand = [rng.randrange(R) for _ in range(18)]
    d.update(kw)
    for k, v in (at or {}).items():
        rand[k] = v
    return d, rand


def make(K, bases, d, rand):
    return RV.prove(K, bases, d["m"], d["r"], rand, d["c_dleq"], d["c"], d["rho"])


def run_calls(cc, gpu, slot, made):
    ob, rb, cb, hb, db = RV.pack(made)
    G = cc.Groth16
    commit = G.range_commit_batch_packed(gpu, slot, ob, rb)
    quotient = G.range_quotient_batch_packed(gpu, ob, rb, cb)
    opened = G.range_open_batch_packed(gpu, ob, rb, cb, hb)
    readable = bytes(1 if x.ok[0] and x.c_dleq < R else 2 for x in made)     # the responses read c_dleq too
    s = G.range_respond_batch(ob, rb, db, status=readable)
    return commit, quotient, opened, s


def compare(made, got, names=None):
    """every output row of the three calls and of the responses against the restatement's bytes"""
    (com_f, com_g, ts, st1), (com_q, ts_q, st2), (evals, proofs, st3), s = got
    for i, x in enumerate(made):
        what = names[i] if names else i
        w_f, w_g, w_ts = RV.expected_commit(x)
        w_q, w_tsq = RV.expected_quotient(x)
        w_ev, w_pr = RV.expected_open(x)
        print("%s: status %d %d %d\n  com_f %s\n  ts %s\n  com_q %s\n  evals %s" % (what, st1[i], st2[i], st3[i], com_f[i].tobytes().hex(),
                                                                                 ts[i].tobytes().hex(), com_q[i].tobytes().hex(), evals[i].tobytes().hex()))
        assert [st1[i], st2[i], st3[i]] == [RV.MADE if ok else RV.MALFORMED for ok in x.ok], what
        assert com_f[i].tobytes() == w_f, what
        assert com_g[i].tobytes() == w_g, what
        assert ts[i].tobytes() == w_ts, what
        assert com_q[i].tobytes() == w_q and ts_q[i].tobytes() == w_tsq, what
        assert evals[i].tobytes() == w_ev, what
        assert proofs[i].tobytes() == w_pr, what
        assert s[i].tobytes() == (RV.fes(x.s) if x.s else bytes(192)), what


def assemble(got, made, i):
    (com_f, com_g, ts, _), (com_q, _, _), (evals, proofs, _), s = got
    flat = [int.from_bytes(s[i, j].tobytes(), "little") for j in range(6)]
    return RV.ark_bytes(com_f[i].tobytes(), com_g[i].tobytes(), evals[i].tobytes(), proofs[i].tobytes(), com_q[i].tobytes(), made[i].c_dleq, flat)


@pytest.mark.parametrize("batch", [1, 3, 65])
def test_every_output_equals_the_restatement_at_4_bits(cc, key4, batch):
    K, gpu, slot = key4
    rng = random.Random(100 + batch)
    made = [make(K, bases_of(), *draw(rng, 4)) for _ in range(batch)]
    compare(made, run_calls(cc, gpu, slot, made))


def test_a_batch_that_spans_two_chunks(cc, key4):
    """CHUNK + 5 showings, five distinct ones in turn: the second chunk starts at the right rows of every array"""
    K, gpu, slot = key4
    rng = random.Random(7)
    kinds = [make(K, bases_of(), *draw(rng, 4)) for _ in range(4)] + [make(K, bases_of(), *draw(rng, 4, m=16))]      # one malformed
    n = CHUNK + 5
    made = [kinds[i % 5] for i in range(n)]
    got = run_calls(cc, gpu, slot, made)
    compare(kinds, tuple(tuple(a[:5] for a in part) for part in got[:3]) + (got[3][:5],))
    for part in got[:3] + ((got[3],),):
        for a in part:
            rows = a.reshape(n, -1)
            want = np.tile(rows[:5], (n // 5 + 1, 1))[:n]
            bad = np.nonzero((rows != want).any(axis=1))[0]
            assert bad.size == 0, "row %d differs from row %d" % (bad[0], bad[0] % 5)


def test_32_bits_where_a_point_has_more_than_64_terms(cc):
    K = RV.key(32)
    rng = random.Random(32)
    bases = bases_of()
    made = [make(K, bases, *draw(rng, 32)), make(K, bases, *draw(rng, 32, m=(1 << 32) - 1))]
    with cc.RangeProofKey(K.data, 32) as gpu:
        slot = gpu.add_bases(*[o.g1_uncompressed(P) for P in bases])
        got = run_calls(cc, gpu, slot, made)
    compare(made, got)
    ped = RV.msm(bases, [made[0].m, made[0].r])
    assert RV.verify(K, bases, ped, assemble(got, made, 0), made[0].c, made[0].rho, got[0][2][0].tobytes()[64:])


def test_2_bits_the_smallest_domain(cc):
    K = RV.key(2)
    rng = random.Random(2)
    bases = bases_of()
    made = [make(K, bases, *draw(rng, 2, m=m)) for m in (0, 1, 2, 3)] + [make(K, bases, *draw(rng, 2, m=4))]
    with cc.RangeProofKey(K.data, 2) as gpu:
        slot = gpu.add_bases(*[o.g1_uncompressed(P) for P in bases])
        got = run_calls(cc, gpu, slot, made)
    compare(made, got)
    assert made[4].ok == (False, False, False)
    ped = RV.msm(bases, [made[3].m, made[3].r])
    assert RV.verify(K, bases, ped, assemble(got, made, 3), made[3].c, made[3].rho, got[0][2][3].tobytes()[64:])


def test_round_trip_through_show_range_batch(cc, key4):
    """the three phases and the responses through the public entry: the assembled RangeProof passes verify_n_bits'
    restatement under the challenges the callable handed out"""
    K, gpu, slot = key4
    rng = random.Random(11)
    openings = [(rng.randrange(16), rng.randrange(R)) for _ in range(3)]
    seen = {}

    def challenge(phase, i, data):
        data = np.asarray(data)
        assert data.shape == {"dleq": (4, 32), "c": (2, 32), "rho": (32,)}[phase]
        seen[phase, i] = (rng.randrange(R), data.tobytes())
        return seen[phase, i][0]

    proofs = cc.Groth16.show_range_batch(gpu, slot, openings, challenge)
    assert len(proofs) == 3 and len(seen) == 9
    bases = bases_of()
    for i, (p, (m, r)) in enumerate(zip(proofs, openings)):
        c_dleq, ts = seen["dleq", i]
        assert p.dleq_c == c_dleq and seen["c", i][1] == ts[:64]
        assert seen["rho", i][1] == o.g1_compressed(RV._rd_g1(p.com_q))
        assert RV.verify(K, bases, RV.msm(bases, [m, r]), p.to_bytes(), seen["c", i][0], seen["rho", i][0], ts[64:]), i
        assert not RV.verify(K, bases, RV.msm(bases, [m ^ 1, r]), p.to_bytes(), seen["c", i][0], seen["rho", i][0], ts[64:]), i
    with pytest.raises(ValueError, match="opening 1 is malformed"):
        cc.Groth16.show_range_batch(gpu, slot, [(3, 5), (16, 5)], challenge)
    assert cc.Groth16.show_range_batch(gpu, slot, [], challenge) == []


@pytest.mark.parametrize("which", [RV.G.start, RV.Q.start + 1, RV.B.start + 2, RV.F.start])
def test_a_rand_value_flipped_in_the_open_call_only_fails_verification(cc, key4, which):
    K, gpu, slot = key4
    rng = random.Random(13 + which)
    bases = bases_of()
    d, rand = draw(rng, 4)
    x = make(K, bases, d, rand)
    ob, rb, cb, hb, db = RV.pack([x])
    G = cc.Groth16
    commit, quotient = G.range_commit_batch_packed(gpu, slot, ob, rb), G.range_quotient_batch_packed(gpu, ob, rb, cb)
    s = G.range_respond_batch(ob, rb, db)
    ped = RV.msm(bases, [x.m, x.r])
    flipped = list(rand)
    flipped[which] ^= 1
    for row, accepted in ((rand, True), (flipped, False)):
        opened = G.range_open_batch_packed(gpu, ob, RV.fes(row), cb, hb)
        assert opened[2][0] == RV.MADE
        proof = assemble((commit, quotient, opened, s), [x], 0)
        assert RV.verify(K, bases, ped, proof, x.c, x.rho, commit[2][0].tobytes()[64:]) == accepted


def edge_rows(K):
    """(name, d, rand) at 4 bits on the key and bases whose scalars are known"""
    n = 4
    rng = random.Random(17)
    w = o.root_of_unity(n)
    beta, s_g, s_gam = K.beta, K.s_g, K.s_gamma
    rows = []

    def case(name, at=None, **kw):
        rows.append((name,) + draw(rng, n, at, **kw))

    case("m = 0", m=0)
    case("m = 2^n - 1", m=15)
    case("m = 2^n", m=16)
    case("m = r", m=R)
    case("a scalar equal to r", at={RV.TR: R})
    case("the opening's r equal to r", r=R)
    case("rand_f all zero", at={3: 0, 4: 0, 5: 0})
    case("rand_g all zero", at={11: 0, 12: 0, 13: 0, 14: 0})
    case("rand_q all zero", at={15: 0, 16: 0, 17: 0})
    case("rand_f zero but f2", at={3: 0, 4: 0})
    case("rho = w", rho=w)
    case("rho = 1", rho=1)
    case("rho = r", rho=R)
    case("c = r", c=R)
    case("c = 0", c=0)
    case("c = 1, rho = 2", c=1, rho=2)
    case("blinding b = (0, 0, 0)", at={0: 0, 1: 0, 2: 0})
    case("blinding b = (0, 0, 1), m = 0", m=0, at={0: 0, 1: 0, 2: 1})
    # com_f = O: m s_g + (f0 + f1 beta + f2 beta^2) s_gamma = 0
    d, rand = draw(rng, n)
    rand[3] = (-(d["m"] * s_g * inv(s_gam)) - rand[4] * beta - rand[5] * beta * beta) % R
    rows.append(("com_f = O", d, rand))
    # k_0 = O: t_m b_0 + t_r b_1 = 0
    d, rand = draw(rng, n)
    rand[RV.TR] = (-rand[RV.TM] * B0 * inv(B1)) % R
    rows.append(("k_0 = O", d, rand))
    # k_1 = O: (t_f0 + t_f1 beta + t_f2 beta^2) s_gamma + t_m s_g = 0
    d, rand = draw(rng, n)
    rand[8] = (-(rand[RV.TM] * s_g * inv(s_gam)) - rand[9] * beta - rand[10] * beta * beta) % R
    rows.append(("k_1 = O", d, rand))
    # f_coeff rand_f + q_coeff rand_q = 0: rand_f = -(rho - 1) rand_q (the random_v deviation of the header)
    d, rand = draw(rng, n)
    rand[RV.F] = [(-(d["rho"] - 1) * x) % R for x in rand[RV.Q]]
    rows.append(("rand_w_hat = 0", d, rand))
    case("every window 0xFF as g0 and as t_m", at={11: M.ALL_FF, RV.TM: M.ALL_FF})
    case("every window 0xFF as q1, b1 and r", r=M.ALL_FF, at={16: M.ALL_FF, 1: M.ALL_FF})
    # equal partials, a doubling inside a point's sum: t_m B_0 = t_r B_1, the two terms of k_0 ...
    d, rand = draw(rng, n)
    rand[RV.TR] = rand[RV.TM] * B0 * inv(B1) % R
    rows.append(("t_m B_0 = t_r B_1", d, rand))
    # ... and deep inside com_g's: the sum of its first n + 4 terms equals the next one, g1 gamma_g[1]
    d, rand = draw(rng, n)
    g = RV.g_blinded(n, d["m"], rand[RV.B])
    so_far = (sum(x * pow(beta, i, R) for i, x in enumerate(g)) * s_g + rand[11] * s_gam) % R
    rand[12] = so_far * inv(s_gam * beta) % R
    rows.append(("com_g's running sum = g1 gamma_g_1", d, rand))
    # ... and opposite ones: the running sum cancels to O and the last two terms start again
    d, rand = draw(rng, n)
    g = RV.g_blinded(n, d["m"], rand[RV.B])
    so_far = (sum(x * pow(beta, i, R) for i, x in enumerate(g)) * s_g + rand[11] * s_gam) % R
    rand[12] = (-so_far * inv(s_gam * beta)) % R
    rows.append(("com_g's running sum = -g1 gamma_g_1", d, rand))
    return rows


def test_edges_between_ordinary_rows(cc, key4):
    K, gpu, slot = key4
    bases = bases_of()
    ordinary = make(K, bases, *draw(random.Random(19), 4))
    edges = edge_rows(K)
    made, names = [ordinary], ["ordinary 0"]
    for name, d, rand in edges:
        made += [make(K, bases, d, rand), ordinary]
        names += [name, "ordinary after " + name]
    got = run_calls(cc, gpu, slot, made)
    compare(made, got, names)
    by_name = {name: (made[1 + 2 * i], 1 + 2 * i) for i, (name, _, _) in enumerate(edges)}
    # the vectors are what they claim to be
    for name, ok in (("m = 2^n", (False,) * 3), ("a scalar equal to r", (False,) * 3), ("rand_f all zero", (False,) * 3),
                     ("rho = w", (True, True, False)), ("rho = 1", (True, True, False)), ("c = r", (True, False, False)),
                     ("rand_f zero but f2", (True,) * 3), ("c = 0", (True,) * 3)):
        assert by_name[name][0].ok == ok, name
    x, i = by_name["com_f = O"]
    assert x.com_f is None and got[0][0][i].tobytes() == bytes(63) + b"\x40" and got[0][2][i, 0].tobytes() == bytes(31) + b"\x40"
    assert by_name["k_0 = O"][0].k[0] is None and by_name["k_1 = O"][0].k[1] is None
    x, i = by_name["rand_w_hat = 0"]
    assert x.vs[2] == 0 and got[2][1][i, 2, 64:].tobytes() == bytes(32) and x.vs[0] and x.vs[1]
    x, i = by_name["blinding b = (0, 0, 0)"]
    assert RV.polys(4, x.m, x.rand).g[4:] == [0, 0, 0]
    # and the made ones verify
    for name in ("m = 0", "m = 2^n - 1", "c = 0", "blinding b = (0, 0, 0)", "com_f = O", "k_0 = O", "rand_w_hat = 0", "t_m B_0 = t_r B_1",
                 "com_g's running sum = g1 gamma_g_1", "com_g's running sum = -g1 gamma_g_1", "every window 0xFF as g0 and as t_m"):
        x, i = by_name[name]
        assert RV.verify(K, bases, RV.msm(bases, [x.m, x.r]), assemble(got, made, i), x.c, x.rho, got[0][2][i].tobytes()[64:]), name


def test_two_slots_on_one_handle(cc, key4):
    K, gpu, slot = key4
    other = bases_of(B0 + 1, B1 + 1)
    slot2 = gpu.add_bases(*[o.g1_uncompressed(P) for P in other])
    assert slot2 != slot
    d, rand = draw(random.Random(23), 4)
    a, b = make(K, bases_of(), d, rand), make(K, other, d, rand)
    ob, rb, _, _, _ = RV.pack([a])
    got_a = cc.Groth16.range_commit_batch_packed(gpu, slot, ob, rb)
    got_b = cc.Groth16.range_commit_batch_packed(gpu, slot2, ob, rb)
    for x, got in ((a, got_a), (b, got_b)):
        w_f, w_g, w_ts = RV.expected_commit(x)
        assert got[0][0].tobytes() == w_f and got[1][0].tobytes() == w_g and got[2][0].tobytes() == w_ts
    assert got_a[0].tobytes() == got_b[0].tobytes()                       # com_f does not look at the slot
    assert got_a[2][0, 2].tobytes() != got_b[2][0, 2].tobytes()           # k_0 does
    assert got_a[2][0, 3].tobytes() == got_b[2][0, 3].tobytes()


def test_the_slot_limit_and_the_last_slot(cc):
    """A key takes 64 slots (csrc/key_handle.hpp, PedersenSlots::MAX_SLOTS): the 65th registration is an argument error, and
    a commitment on slot 63 is the one slot 0 makes when both hold the same bases."""
    K = RV.key(4)
    pair = [o.g1_uncompressed(P) for P in bases_of()]
    with cc.RangeProofKey(K.data, 4) as gpu:
        assert [gpu.add_bases(*pair) for _ in range(64)] == list(range(64))
        with pytest.raises(cc.CrescentGpuError, match="slots of this key are taken") as e:
            gpu.add_bases(*pair)
        assert e.value.code == INVALID_ARGUMENT
        x = make(K, bases_of(), *draw(random.Random(24), 4))
        ob, rb, _, _, _ = RV.pack([x])
        first = cc.Groth16.range_commit_batch_packed(gpu, 0, ob, rb)
        last = cc.Groth16.range_commit_batch_packed(gpu, 63, ob, rb)
    w_f, w_g, w_ts = RV.expected_commit(x)
    assert first[0][0].tobytes() == w_f and first[1][0].tobytes() == w_g and first[2][0].tobytes() == w_ts and first[3][0] == RV.MADE
    for a, b in zip(first, last):
        assert a.tobytes() == b.tobytes()


def test_argument_errors_under_a_handle(cc, key4):
    K, gpu, slot = key4
    L = cc.lib()
    buf = (ctypes.c_uint8 * 4096)()
    h = gpu._h
    assert L.cg_range_commit_batch(h, 63, buf, buf, 1, buf, buf, buf, buf) == INVALID_ARGUMENT          # a slot nobody registered
    assert b"slot 63" in L.cg_last_error()
    assert L.cg_range_commit_batch(h, 63, buf, buf, 0, buf, buf, buf, buf) == INVALID_ARGUMENT
    for i in (2, 3, 5, 6, 7, 8):
        args = [h, slot, buf, buf, 1, buf, buf, buf, buf]
        args[i] = None
        assert L.cg_range_commit_batch(*args) == INVALID_ARGUMENT, i
    for i in (1, 2, 3, 5, 6, 7):
        args = [h, buf, buf, buf, 1, buf, buf, buf]
        args[i] = None
        assert L.cg_range_quotient_batch(*args) == INVALID_ARGUMENT, i
    for i in (1, 2, 3, 4, 6, 7, 8):
        args = [h, buf, buf, buf, buf, 1, buf, buf, buf]
        args[i] = None
        assert L.cg_range_open_batch(*args) == INVALID_ARGUMENT, i
    assert b"null" in L.cg_last_error()
    assert L.cg_range_commit_batch(h, slot, None, None, 0, None, None, None, None) == 0                 # n = 0
    assert L.cg_range_quotient_batch(h, None, None, None, 0, None, None, None) == 0
    assert L.cg_range_open_batch(h, None, None, None, None, 0, None, None, None) == 0
    s = ctypes.c_uint32()
    off_curve = bytearray(bases_bytes(bases_of()))
    off_curve[0] ^= 1
    assert L.cg_range_pk_add_bases(h, bytes(off_curve), ctypes.byref(s)) == INVALID_ARGUMENT
    not_canonical = RV.fe(o.Q) + bytes(off_curve[32:])
    assert L.cg_range_pk_add_bases(h, not_canonical, ctypes.byref(s)) == INVALID_ARGUMENT
