"""Range proofs in one call each way (csrc/rangeproof.hip: cg_range_prove_batch; csrc/rangeverify.hip:
cg_range_verify_proofs_batch), the Merlin transcripts on the GPU (csrc/merlin.hpp).  The prover is compared byte for byte
with the three-call path driven by the pure-Python Merlin of tests/merlin_vectors.py, and its proofs are checked by the
restatement of `verify_n_bits`; the verifier is compared with cg_range_verify_batch driven by the same Python Merlin and with
the trapdoor oracle of tests/range_verify_vectors.py plus the Python challenge comparison."""
import ctypes
import random

import numpy as np
import pytest

import merlin_vectors as MV
import range_vectors as RV
import range_verify_vectors as V

pytestmark = pytest.mark.gpu

o = RV.o
R, Q = V.R, V.Q
ACCEPT, REJECT, MALFORMED = V.ACCEPT, V.REJECT, V.MALFORMED
MADE, NOT_MADE = 1, 2
INVALID_ARGUMENT = -1
RCHUNK, RVCHUNK = 1 << 12, 1 << 15           # showings per launch set (csrc/rangeproof.hip, csrc/rangeverify.hip)
unc, cmp = o.g1_uncompressed, o.g1_compressed
fe, fes = RV.fe, RV.fes
BASES = V.bases_of()
OTHER_BASES = V.bases_of(0x777, 0x999)


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()
    assert cc.CG_SHOW_MADE == MADE and cc.CG_SHOW_MALFORMED == NOT_MADE


_keys = {}


@pytest.fixture(scope="module")
def keys(cc):
    """per n_bits: (K, proving key, its slot, verifying key, its slot, a second slot with other bases), made on demand"""
    def get(n_bits):
        if n_bits not in _keys:
            K = RV.key(n_bits)
            pk = cc.RangeProofKey(K.data, n_bits)
            vk = cc.RangeVerifyingKey(V.vk_bytes(K), n_bits)
            pair, other = [unc(P) for P in BASES], [unc(P) for P in OTHER_BASES]
            _keys[n_bits] = (K, pk, pk.add_bases(*pair), vk, vk.add_bases(*pair), vk.add_bases(*other))
        return _keys[n_bits]
    yield get
    for _, pk, _, vk, _, _ in _keys.values():
        pk.close()
        vk.close()
    _keys.clear()


def compress(b):
    from crescent_credentials_amd import api
    return api._g1_compress(b).tobytes()


class Host:
    """the host's Merlin of show_range_batch / verify_range_batch: tests/merlin_vectors.py over the bytes they pass"""

    def __init__(self, K, peds, bases=BASES):
        self.slot = [cmp(B) for B in bases]
        self.cfb = [cmp(P) for P in K.pgam[:3] + [K.pg[0]]]
        self.peds = [compress(p) for p in peds]
        self.fg = {}

    def __call__(self, phase, i, data):
        d = np.asarray(data)
        if phase == "c":
            self.fg[i] = (d[0].tobytes(), d[1].tobytes())
            t = MV.new_transcript()
            t.append_message(b"com_f", self.fg[i][0])
            t.append_message(b"com_g", self.fg[i][1])
            return MV.to_int(MV.challenge(t))
        if phase == "rho":
            return MV.to_int(MV.range_challenges(self.fg[i][0], self.fg[i][1], d.tobytes())[1])
        assert phase == "dleq" and d.shape == (4, 32)
        return MV.to_int(MV.range_dleq_challenge(self.slot, self.cfb, d[2].tobytes(), d[3].tobytes(), self.peds[i], d[0].tobytes()))


def three_calls(cc, pk, slot, ob, rb, host, n):
    """the existing path on packed arrays; a showing some call reports malformed stays zero from there on"""
    G = cc.Groth16
    com_f, com_g, ts, st = G.range_commit_batch_packed(pk, slot, ob, rb)
    made = st == MADE
    c_dleq = [host("dleq", i, ts[i]) if made[i] else 0 for i in range(n)]
    cs = [host("c", i, ts[i, :2]) if made[i] else 0 for i in range(n)]
    com_q, ts_q, st = G.range_quotient_batch_packed(pk, ob, rb, fes(cs))
    assert list(st == MADE) == list(made)
    rhos = [host("rho", i, ts_q[i]) if made[i] else 0 for i in range(n)]
    evals, proofs, st = G.range_open_batch_packed(pk, ob, rb, fes(cs), fes(rhos))
    assert list(st == MADE) == list(made)
    s = G.range_respond_batch(ob, rb, fes(c_dleq), st)
    chal = b"".join(fe(a) + fe(b) + fe(c) for a, b, c in zip(c_dleq, cs, rhos))
    return [com_f.tobytes(), com_g.tobytes(), com_q.tobytes(), evals.tobytes(), proofs.tobytes(), fes(c_dleq), s.tobytes(), chal, st.tobytes()]


NAMES = ["com_f", "com_g", "com_q", "evals", "proofs", "pok_c", "pok_s", "challenges", "status"]
WIDTH = [64, 64, 64, 96, 288, 32, 192, 96, 1]


def rows_of(arrays, i):
    return [bytes(a)[w * i:w * (i + 1)] for a, w in zip(arrays, WIDTH)]


def draw(rng, n_bits, n):
    openings = [(rng.randrange(1 << n_bits), rng.randrange(R)) for _ in range(n)]
    rand = [[rng.randrange(R) for _ in range(RV.N_RAND)] for _ in range(n)]
    return openings, rand


def pack_in(openings, rand):
    return b"".join(fe(m) + fe(r) for m, r in openings), b"".join(fes(row) for row in rand)


@pytest.mark.parametrize("n_bits", [2, 4, 32])
@pytest.mark.parametrize("batch", [1, 5, 65])
def test_one_call_equals_the_three_calls(cc, keys, n_bits, batch):
    """every output byte, the challenges included; at 5, rows 1 and 3 are malformed in different ways"""
    K, pk, slot, _, _, _ = keys(n_bits)
    rng = random.Random(1000 * n_bits + batch)
    openings, rand = draw(rng, n_bits, batch)
    peds = [unc(RV.msm(BASES, [m, r])) for m, r in openings]
    bad = []
    if batch == 5:
        openings[1] = (1 << n_bits, openings[1][1])                                # m >= 2^n_bits
        off = bytearray(peds[3])
        off[0] ^= 1
        assert not V.rd_g1_checked(bytes(off))[0]
        peds[3] = bytes(off)                                                       # ped_com off the curve
        bad = [1, 3]
    ob, rb = pack_in(openings, rand)
    got = [a.tobytes() for a in cc.Groth16.range_prove_batch_packed(pk, slot, ob, b"".join(peds), rb)]
    want = three_calls(cc, pk, slot, ob, rb, Host(K, peds), batch)
    for i in range(batch):
        g, w = rows_of(got, i), rows_of(want, i)
        for name, a, b in zip(NAMES, g, w):
            if i in bad:
                assert a == (bytes([NOT_MADE]) if name == "status" else bytes(len(a))), (i, name)
            else:
                assert a == b, (i, name, a.hex()[:64], b.hex()[:64])
        if i not in bad:
            assert g[8] == bytes([MADE]) and g[7][:32] == g[5] and g[7][31] == g[7][63] == g[7][95] == 0
    if bad:                                                                        # the neighbours, against a batch without the two
        keep = [i for i in range(batch) if i not in bad]
        ob2, rb2 = pack_in([openings[i] for i in keep], [rand[i] for i in keep])
        alone = [a.tobytes() for a in cc.Groth16.range_prove_batch_packed(pk, slot, ob2, b"".join(peds[i] for i in keep), rb2)]
        for j, i in enumerate(keep):
            assert rows_of(alone, j) == rows_of(got, i), i


def test_one_past_a_chunk_of_the_prover(cc, keys):
    """4097 showings at n_bits = 2, tiled from four openings: a per-call index into a per-chunk buffer shows in the second
    chunk, whose rows 4095 (the first chunk's last) and 4096 must equal their twins"""
    K, pk, slot, _, _, _ = keys(2)
    n = RCHUNK + 1
    rng = random.Random(77)
    openings, rand = draw(rng, 2, 4)
    peds = [unc(RV.msm(BASES, [m, r])) for m, r in openings]
    ob, rb = pack_in(openings, rand)
    tile = lambda b, w: (np.frombuffer(b, np.uint8).reshape(4, w)[np.arange(n) % 4]).copy()
    first = cc.Groth16.range_prove_batch_packed(pk, slot, ob, b"".join(peds), rb)
    assert list(first[8]) == [MADE] * 4
    want = three_calls(cc, pk, slot, ob, rb, Host(K, peds), 4)
    assert [a.tobytes() for a in first] == want
    got = cc.Groth16.range_prove_batch_packed(pk, slot, tile(ob, 64), tile(b"".join(peds), 64), tile(rb, 32 * RV.N_RAND))
    for name, a, f in zip(NAMES, got, first):
        a, f = a.reshape(n, -1), f.reshape(4, -1)
        for i in (0, 3, RCHUNK - 1, RCHUNK):
            assert a[i].tobytes() == f[i % 4].tobytes(), (name, i)
        assert (a == f[np.arange(n) % 4]).all(), name


def proofs_of(cc, got, i):
    """showing i of range_prove_batch_packed's arrays as the pieces the oracles take"""
    com_f, com_g, com_q, evals, proofs, pok_c, pok_s, chal, status = got
    val = lambda a: int.from_bytes(a.tobytes(), "little")
    return dict(com_f=com_f[i].tobytes(), com_g=com_g[i].tobytes(), com_q=com_q[i].tobytes(), evals=[val(evals[i, j]) for j in range(3)],
                W=[proofs[i, j, :64].tobytes() for j in range(3)], vs=[val(proofs[i, j, 64:]) for j in range(3)], pok_c=val(pok_c[i]),
                s=[val(pok_s[i, j]) for j in range(6)], chal=[val(chal[i, j]) for j in range(3)])


def row_of(p, ped, r1, r2):
    return V.Row(ped, p["com_f"], p["com_g"], p["com_q"], p["evals"], p["W"], p["vs"], p["chal"][1], p["chal"][2], r1, r2, p["pok_c"], p["s"])


@pytest.fixture(scope="module")
def made4(cc, keys):
    """six proofs of the one-call prover at n_bits = 4, as rows with randomizers; shared, and left as they are"""
    K, pk, slot, _, _, _ = keys(4)
    rng = random.Random(300)
    openings, rand = draw(rng, 4, 6)
    peds = [unc(RV.msm(BASES, [m, r])) for m, r in openings]
    ob, rb = pack_in(openings, rand)
    got = cc.Groth16.range_prove_batch_packed(pk, slot, ob, b"".join(peds), rb)
    assert list(got[8]) == [MADE] * 6
    rows = [row_of(proofs_of(cc, got, i), peds[i], rng.getrandbits(128), rng.getrandbits(128)) for i in range(6)]
    return rows, openings, rand


def merlin_of(x):
    """(c, rho) of the row's commitments as their bytes compress"""
    c, rho = MV.range_challenges(compress(x.com_f), compress(x.com_g), compress(x.com_q))
    return MV.to_int(c), MV.to_int(rho)


def oracle_verdict(K, x, bases=BASES):
    """verify_n_bits: the trapdoor oracle under the Merlin challenges, then the DLEQ's challenge compared with pok_c"""
    c, rho = merlin_of(x)
    verdict, k = V.expected(K, bases, x.but(c=c, rho=rho))
    if verdict != ACCEPT:
        return verdict
    cfb = [cmp(P) for P in K.pgam[:3] + [K.pg[0]]]
    c_dleq = MV.range_dleq_challenge([cmp(B) for B in bases], cfb, k[:32], k[32:], compress(x.ped_com), compress(x.com_f))
    return ACCEPT if MV.to_int(c_dleq) == x.pok_c else REJECT


def test_proofs_satisfy_the_verification_identities(made4, keys):
    """three proofs against the pure-Python verify_n_bits of tests/range_vectors.py, the challenges from the Python Merlin"""
    K = keys(4)[0]
    rows, openings, _ = made4
    for x, (m, r) in list(zip(rows, openings))[:3]:
        c, rho = merlin_of(x)
        assert (c, rho) == (x.c, x.rho)                                            # challenges_out
        proof = RV.ark_bytes(x.com_f, x.com_g, fes(x.evals), b"".join(W + fe(v) for W, v in zip(x.W, x.vs)), x.com_q, x.pok_c, x.s)
        assert RV.verify(K, BASES, RV.msm(BASES, [m, r]), proof, c, rho)
        assert not RV.verify(K, BASES, RV.msm(BASES, [m, r]), proof, c ^ 1, rho)
        assert oracle_verdict(K, x) == ACCEPT                                      # the DLEQ's challenge over the recomputed k


def as_range_proof(cc, x):
    return cc.RangeProof(x.com_f, x.com_g, x.evals[0], x.W[0] + fe(x.vs[0]), x.evals[1], x.W[1] + fe(x.vs[1]), x.com_q, x.evals[2],
                         x.W[2] + fe(x.vs[2]), x.pok_c, [x.s[:2], x.s[2:]])


def run_verify(cc, vk, slot, rows):
    a = V.pack(rows)
    return list(cc.Groth16.range_verify_proofs_batch_packed(vk, slot, *a[:6], a[8], a[9], a[10]))


def negated(b):
    y = int.from_bytes(b[32:63] + bytes([b[63] & 0x3F]), "little")
    return b[:32] + o.g1_uncompressed((int.from_bytes(b[:32], "little"), (Q - y) % Q))[32:]


@pytest.fixture(scope="module")
def seven(made4, keys):
    """a valid proof and six ways to spoil one, with the verdict verify_n_bits gives"""
    K = keys(4)[0]
    rows, openings, _ = made4
    rng = random.Random(301)
    x = rows[0]
    m, r = openings[0]
    off = bytearray(x.com_q)
    off[0] ^= 1
    cases = [("valid", x, ACCEPT),
             ("pok_c with one bit flipped", x.but(pok_c=x.pok_c ^ (1 << 100)), REJECT),
             ("ped_com of another opening", x.but(ped_com=unc(RV.msm(BASES, [m ^ 1, r]))), REJECT),
             ("com_q another point", x.but(com_q=unc(RV.g1(rng.randrange(R)))), REJECT),
             ("com_g negated", x.but(com_g=negated(x.com_g)), REJECT),
             ("com_q off the curve", x.but(com_q=bytes(off)), MALFORMED),
             ("s_00 != s_13", x.with_item("s", 5, (x.s[5] + 1) % R), REJECT)]
    assert compress(cases[4][1].com_g)[:31] == compress(x.com_g)[:31] and compress(cases[4][1].com_g)[31] ^ compress(x.com_g)[31] == 0x80
    # the other opening's commitment leaves the group stage accepting: only the challenge comparison sees it
    y = cases[2][1]
    assert V.expected(K, BASES, y)[0] == ACCEPT
    for name, row, verdict in cases:
        assert oracle_verdict(K, row) == verdict, name
    return cases


@pytest.mark.parametrize("latency", [False, True])
def test_verdicts_equal_the_two_call_path_and_the_oracle(cc, keys, made4, seven, latency):
    K, _, _, vk, slot, _ = keys(4)
    rows = [row for _, row, _ in seven]
    want = [verdict for _, _, verdict in seven]
    vk.set_latency(latency)
    try:
        got = run_verify(cc, vk, slot, rows)
        assert got == want, [name for (name, _, _), g, w in zip(seven, got, want) if g != w]
        assert run_verify(cc, vk, slot, rows[:1]) == [ACCEPT]                      # a batch of one
        assert run_verify(cc, vk, slot, made4[0]) == [ACCEPT] * 6
        # the neighbours of the malformed row, and the order, do not matter
        assert run_verify(cc, vk, slot, rows[::-1]) == want[::-1]
        if not latency:
            host = Host(K, [x.ped_com for x in rows])
            two_call = cc.Groth16.verify_range_batch(vk, slot, [x.ped_com for x in rows], [as_range_proof(cc, x) for x in rows], host,
                                                     [(x.r1, x.r2) for x in rows])
            assert two_call == [v == ACCEPT for v in want]
    finally:
        vk.set_latency(False)


def test_one_past_a_chunk_of_the_verifier(cc, keys):
    """32769 proofs at n_bits = 2, tiled from four the one-call prover made; the last row of the first chunk and the only
    row of the second are spoiled"""
    K, pk, slot, vk, vslot, _ = keys(2)
    n = RVCHUNK + 1
    rng = random.Random(302)
    openings, rand = draw(rng, 2, 4)
    peds = [unc(RV.msm(BASES, [m, r])) for m, r in openings]
    ob, rb = pack_in(openings, rand)
    got = cc.Groth16.range_prove_batch_packed(pk, slot, ob, b"".join(peds), rb)
    assert list(got[8]) == [MADE] * 4
    rows = [row_of(proofs_of(cc, got, i), peds[i], rng.getrandbits(128), rng.getrandbits(128)) for i in range(4)]
    spoiled = {RVCHUNK - 1: rows[(RVCHUNK - 1) % 4].but(pok_c=rows[(RVCHUNK - 1) % 4].pok_c ^ 1),
               RVCHUNK: rows[RVCHUNK % 4].but(com_q=unc(RV.g1(rng.randrange(R))))}
    for x in list(rows) + list(spoiled.values()):
        assert oracle_verdict(K, x) == (ACCEPT if x in rows else REJECT)
    a = V.pack(rows)
    idx = np.arange(n) % 4
    arrays = []
    for j, b in enumerate(a):
        t = np.frombuffer(b, np.uint8).reshape(4, -1)[idx].copy()
        for i, x in spoiled.items():
            t[i] = np.frombuffer(V.pack([x])[j], np.uint8)
        arrays.append(t)
    verdicts = cc.Groth16.range_verify_proofs_batch_packed(vk, vslot, *arrays[:6], arrays[8], arrays[9], arrays[10])
    want = np.full(n, ACCEPT, np.uint8)
    want[list(spoiled)] = REJECT
    assert verdicts[RVCHUNK - 1] == REJECT and verdicts[RVCHUNK] == REJECT and verdicts[RVCHUNK - 2] == ACCEPT
    assert (verdicts == want).all(), np.nonzero(verdicts != want)[0][:10]


def test_round_trip(cc, keys):
    K, pk, slot, vk, vslot, other_slot = keys(4)
    rng = random.Random(303)
    openings, _ = draw(rng, 4, 3)
    peds = [unc(RV.msm(BASES, [m, r])) for m, r in openings]
    proofs = cc.Groth16.prove_range_batch(pk, slot, openings, peds)               # the package draws the randomness
    assert cc.Groth16.verify_range_proofs(vk, vslot, peds, proofs) == [True] * 3
    assert cc.Groth16.verify_range_proofs(vk, other_slot, peds, proofs) == [False] * 3
    assert cc.Groth16.verify_range_proofs(vk, vslot, peds[1:] + peds[:1], proofs) == [False] * 3
    assert cc.Groth16.prove_range_batch(pk, slot, [], []) == [] and cc.Groth16.verify_range_proofs(vk, vslot, [], []) == []
    with pytest.raises(ValueError, match="opening 1 is malformed"):
        cc.Groth16.prove_range_batch(pk, slot, [openings[0], (16, 5)], peds[:2])


def test_argument_errors_under_a_handle(cc, keys):
    _, pk, slot, vk, vslot, _ = keys(4)
    L = cc.lib()
    buf = (ctypes.c_uint8 * 4096)()
    prove = [pk._h, slot, buf, buf, buf, 1] + [buf] * 9
    assert L.cg_range_prove_batch(*(prove[:1] + [63] + prove[2:])) == INVALID_ARGUMENT                  # a slot nobody registered
    assert b"slot 63" in L.cg_last_error()
    for i in (2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 14):               # every array but challenges_out, which may be left out
        args = list(prove)
        args[i] = None
        assert L.cg_range_prove_batch(*args) == INVALID_ARGUMENT, i
        assert b"null" in L.cg_last_error()
    assert L.cg_range_prove_batch(pk._h, slot, None, None, None, 0, *([None] * 9)) == 0                # n = 0
    verify = [vk._h, vslot] + [buf] * 9 + [1, buf]
    assert L.cg_range_verify_proofs_batch(*(verify[:1] + [63] + verify[2:])) == INVALID_ARGUMENT
    assert b"slot 63" in L.cg_last_error()
    for i in (2, 3, 4, 5, 6, 7, 8, 9, 10, 12):                    # pok_c included: this entry has no mode without a DLEQ
        args = list(verify)
        args[i] = None
        assert L.cg_range_verify_proofs_batch(*args) == INVALID_ARGUMENT, i
        assert b"null" in L.cg_last_error()
    assert L.cg_range_verify_proofs_batch(vk._h, vslot, *([None] * 9), 0, None) == 0                   # n = 0


def test_challenges_out_may_be_left_out(cc, keys):
    K, pk, slot, _, _, _ = keys(4)
    rng = random.Random(304)
    openings, rand = draw(rng, 4, 2)
    peds = b"".join(unc(RV.msm(BASES, [m, r])) for m, r in openings)
    ob, rb = pack_in(openings, rand)
    want = cc.Groth16.range_prove_batch_packed(pk, slot, ob, peds, rb)
    bufs = [np.zeros(2 * w, np.uint8) for w in WIDTH]
    p = lambda a: a.ctypes.data
    i8 = lambda b: np.frombuffer(b, np.uint8).copy()
    a_ob, a_ped, a_rb = i8(ob), i8(peds), i8(rb)
    rc = cc.lib().cg_range_prove_batch(pk._h, slot, p(a_ob), p(a_ped), p(a_rb), 2, *[p(b) for b in bufs[:7]], None, p(bufs[8]))
    assert rc == 0
    for j in (0, 1, 2, 3, 4, 5, 6, 8):
        assert bufs[j].tobytes() == want[j].tobytes(), NAMES[j]
