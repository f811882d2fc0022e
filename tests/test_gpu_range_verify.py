"""Verifying range proofs on the GPU (csrc/rangeverify.hip: cg_range_verify_batch): `RangeProof::verify_n_bits`
(creds/src/rangeproof.rs:342-424) between the host's transcripts, for batches of proofs under one `RangeProofVK`.  Every
verdict and every k_out byte is compared exactly with the trapdoor restatement of tests/range_verify_vectors.py (route
(a)), on proofs the restatement of the prover makes and on forged ones the reference accepts, which make the edge cases
ACCEPT-sensitive."""
import ctypes
import random

import numpy as np
import pytest

import bn254_oracle as o
import range_vectors as RV
import range_verify_vectors as V

pytestmark = pytest.mark.gpu

R, Q = V.R, V.Q
ACCEPT, REJECT, MALFORMED = V.ACCEPT, V.REJECT, V.MALFORMED
INVALID_ARGUMENT = -1
CHUNK = 1 << 15                      # showings per launch set (csrc/rangeverify.hip, RVCHUNK)
unc = V.unc


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


def load(cc, K, bases=None, **kw):
    gpu = cc.RangeVerifyingKey(V.vk_bytes(K, **kw), K.n_bits)
    return gpu, gpu.add_bases(*[unc(P) for P in (bases or V.bases_of())])


@pytest.fixture(scope="module")
def vk4(cc):
    K = RV.key(4)
    gpu, slot = load(cc, K)
    yield K, gpu, slot
    gpu.close()


_memo = {}


def want(K, bases, x, **kw):
    """route (a), once per distinct row"""
    key = (K.n_bits, tuple(V.unc(B) for B in bases), V.pack([x]), tuple(sorted(kw.items())))
    if key not in _memo:
        _memo[key] = V.expected(K, bases, x, **kw)
    return _memo[key]


def run(cc, gpu, slot, rows, pok=True):
    a = V.pack(rows)
    return cc.Groth16.range_verify_batch_packed(gpu, slot, *a) if pok else cc.Groth16.range_verify_batch_packed(gpu, slot, None, *a[1:9])


def check(cc, gpu, slot, K, rows, names=None, bases=None, **kw):
    """every verdict and k_out row against route (a); returns the expected (verdict, k) list"""
    bases = bases or V.bases_of()
    verdicts, k = run(cc, gpu, slot, rows)
    wants = [want(K, bases, x, **kw) for x in rows]
    for i, (x, (w_v, w_k)) in enumerate(zip(rows, wants)):
        what = names[i] if names else i
        print("%s: verdict %d (want %d)  k %s" % (what, verdicts[i], w_v, k[i].tobytes().hex()))
        assert verdicts[i] == w_v, what
        assert k[i].tobytes() == w_k, what
    return wants


@pytest.fixture(scope="module")
def valid(vk4):
    """65 distinct proofs of the prover's restatement with random challenges and randomizers, and the k bytes it absorbed"""
    K, _, _ = vk4
    rng = random.Random(200)
    rows, absorbed = [], []
    for _ in range(65):
        x, made = V.valid_row(K, V.bases_of(), rng)
        rows.append(x)
        absorbed.append(RV.expected_commit(made)[2][64:])
    return rows, absorbed


@pytest.mark.parametrize("batch", [1, 3, 65])
def test_valid_proofs_are_accepted_with_the_absorbed_k(cc, vk4, valid, batch):
    K, gpu, slot = vk4
    rows, absorbed = valid
    wants = check(cc, gpu, slot, K, rows[:batch])
    assert [w[0] for w in wants] == [ACCEPT] * batch
    assert [w[1] for w in wants] == absorbed[:batch]


def interleave(ordinary, cases):
    rows, names = [ordinary[0]], ["ordinary 0"]
    for i, (name, x) in enumerate(cases):
        rows += [x, ordinary[(i + 1) % len(ordinary)]]
        names += [name, "ordinary after " + name]
    return rows, names


def test_one_field_changed_at_a_time(cc, vk4, valid):
    K, gpu, slot = vk4
    rng = random.Random(201)
    x = valid[0][5]
    other = lambda: unc(RV.g1(rng.randrange(R)))
    points = ["ped_com", "com_f", "com_g", "com_q", ("W", 0), ("W", 1), ("W", 2)]

    def point_set(row, where, b):
        return row.with_item(where[0], where[1], b) if isinstance(where, tuple) else row.but(**{where: b})

    def point_get(row, where):
        return getattr(row, where[0])[where[1]] if isinstance(where, tuple) else getattr(row, where)

    def off_curve(b):
        b = bytearray(b)
        b[0] ^= 1
        return bytes(b)

    x_is_q = lambda b: RV.fe(Q) + b[32:]
    y_is_q = lambda b: b[:32] + RV.fe(Q)
    bad_flags = lambda b: b[:63] + bytes([b[63] | 0xC0])
    cases, category = [], {}

    def case(name, row, verdict):
        cases.append((name, row))
        category[name] = verdict

    for where in points:
        case("%s moved" % (where,), point_set(x, where, other()), ACCEPT if where == "ped_com" else REJECT)
    for where, how in zip(points, (off_curve, bad_flags, off_curve, x_is_q, bad_flags, off_curve, y_is_q)):
        case("%s %s" % (where, how.__name__ if hasattr(how, "__name__") else "bad"), point_set(x, where, how(point_get(x, where))), MALFORMED)
    for j in range(3):
        case("eval %d" % j, x.with_item("evals", j, x.evals[j] ^ 1), REJECT)
        case("random_v %d" % j, x.with_item("vs", j, x.vs[j] ^ 1), REJECT)
        case("eval %d = r" % j, x.with_item("evals", j, R), MALFORMED)
        case("random_v %d = r" % j, x.with_item("vs", j, R), MALFORMED)
    case("c", x.but(c=x.c ^ 1), REJECT)
    case("rho", x.but(rho=x.rho ^ 1), REJECT)
    case("c = r", x.but(c=R), MALFORMED)
    case("rho = r", x.but(rho=R), MALFORMED)
    case("pok_c = r", x.but(pok_c=R), MALFORMED)
    case("s_13 != s_00", x.with_item("s", 5, x.s[5] ^ 1), REJECT)
    for j in range(6):
        case("s[%d] = r" % j, x.with_item("s", j, R), MALFORMED)
    case("s_01 changed", x.with_item("s", 1, x.s[1] ^ 1), ACCEPT)
    rows, names = interleave([valid[0][6], valid[0][7]], cases)
    wants = dict(zip(names, check(cc, gpu, slot, K, rows, names)))
    for name, verdict in category.items():
        assert wants[name][0] == verdict, name                     # the vectors are what they claim to be
    assert all(w[0] == ACCEPT for name, w in wants.items() if name.startswith("ordinary"))
    base = want(K, V.bases_of(), x)[1]
    for name in ("ped_com moved", "s_01 changed"):                  # only k_0 changes
        assert wants[name][1][:32] != base[:32] and wants[name][1][32:] == base[32:], name


def test_randomizers_are_used_as_the_reference_uses_them(cc, vk4, valid):
    K, gpu, slot = vk4
    rng = random.Random(202)
    x = valid[0][8]
    keep, lose = V.cancelling_rows(x, rng.randrange(R))
    broken = x.with_item("vs", 1, x.vs[1] ^ 1).with_item("W", 1, unc(RV.g1(rng.randrange(R))))
    top = 2 ** 128 - 1
    cases = [("shifted random_v, r_1", keep), ("shifted random_v, r_1 + 1", lose), ("broken proof_gw, r_1 = 0", broken.but(r1=0)),
             ("broken proof_gw, r_1 = 1", broken.but(r1=1)), ("both randomizers 2^128 - 1", x.but(r1=top, r2=top)),
             ("both randomizers 0", x.but(r1=0, r2=0)), ("broken proof_w^, r_2 = 0", x.with_item("evals", 2, x.evals[2] ^ 1).but(r2=0))]
    rows, names = interleave([valid[0][9]], cases)
    wants = dict(zip(names, check(cc, gpu, slot, K, rows, names)))
    assert [wants[name][0] for name, _ in cases] == [ACCEPT, REJECT, ACCEPT, REJECT, ACCEPT, ACCEPT, REJECT]
    # (a proof_w^ whose evaluation is off fails the identity whatever r_2 is)


def edge_rows(K):
    n = K.n_bits
    rng = random.Random(203)
    w = o.root_of_unity(n)
    wl = pow(w, n - 1, R)
    bases = V.bases_of()
    rows = []
    case = lambda name, x, verdict: rows.append((name, x, verdict))
    case("rho = 1", V.forged_row(K, rng).but(rho=1), MALFORMED)
    case("rho = w^(n-1)", V.forged_row(K, rng).but(rho=wl), MALFORMED)
    x = V.forged_row(K, rng, rho=w)
    assert V.coeffs(n, w) == (0, 0)
    case("forged rho = w: com_w^ = O", x, ACCEPT)
    case("forged rho = w, eval_w^ off", x.with_item("evals", 2, x.evals[2] ^ 1), REJECT)
    case("forged rho = 0", V.forged_row(K, rng, rho=0), ACCEPT)
    case("forged c = 0", V.forged_row(K, rng, c=0), ACCEPT)
    case("real c = 0", V.valid_row(K, bases, rng, c=0)[0], ACCEPT)
    case("all infinity, all zero", V.all_infinity_row(), ACCEPT)
    # com_f = O from a real opening: m s_g + (f0 + f1 beta + f2 beta^2) s_gamma = 0
    m = rng.randrange(1 << n)
    rand = [rng.randrange(R) for _ in range(18)]
    rand[3] = (-(m * K.s_g * V.inv(K.s_gamma)) - rand[4] * K.beta - rand[5] * K.beta * K.beta) % R
    x, made = V.valid_row(K, bases, rng, m=m, rand=rand)
    assert made.com_f is None and x.com_f == unc(None)
    case("com_f = O from a real opening", x, ACCEPT)
    # a doubling inside com_w^'s sum: com_q = com_f, and rho = 2 makes f_coeff = q_coeff
    a = rng.randrange(R)
    assert V.coeffs(n, 2)[0] == V.coeffs(n, 2)[1]
    x = V.forged_row(K, rng, a_f=a, a_q=a, rho=2)
    case("forged com_q = com_f, rho = 2", x, ACCEPT)
    case("forged com_q = com_f, rho = 2, random_v off", x.with_item("vs", 2, x.vs[2] ^ 1), REJECT)
    # the running sum passes through O: com_g = O, then r_2 f_coeff com_f = -(r_2 q_coeff com_q)
    rho = rng.randrange(R)
    q_coeff, f_coeff = V.coeffs(n, rho)
    a = rng.randrange(R)
    x = V.forged_row(K, rng, a_g=0, a_f=a, a_q=(-f_coeff * a * V.inv(q_coeff)) % R, rho=rho)
    case("forged f_coeff com_f = -q_coeff com_q after com_g = O", x, ACCEPT)
    good, bad = V.total_w_zero_rows(K, rng)
    case("forged total_w = O, total_c = O", good, ACCEPT)
    case("forged total_w = O, total_c != O", bad, REJECT)
    ff = 2 ** 248 - 1                                              # every 8-bit window 0xFF, below r
    top = 2 ** 128 - 1
    case("every window 0xFF: responses, pok_c, randomizers", V.forged_row(K, rng, s=[ff] * 6, pok_c=ff, r1=top, r2=top), ACCEPT)
    case("every window 0xFF: rho, c, evaluations, random_v", V.forged_row(K, rng, rho=ff, c=ff, eval_g=ff, eval_gw=ff, vs=[ff] * 3), ACCEPT)
    case("identity off by one, openings valid", V.identity_breaker(K, rng), REJECT)
    return rows


def test_edges_between_ordinary_rows(cc, vk4, valid):
    K, gpu, slot = vk4
    edges = edge_rows(K)
    rows, names = interleave([valid[0][10], valid[0][11]], [(name, x) for name, x, _ in edges])
    wants = dict(zip(names, check(cc, gpu, slot, K, rows, names)))
    for name, _, verdict in edges:
        assert wants[name][0] == verdict, name                     # the vectors are what they claim to be
    assert all(w[0] == ACCEPT for name, w in wants.items() if name.startswith("ordinary"))
    assert wants["all infinity, all zero"][1] == (bytes(31) + b"\x40") * 2


def test_a_key_whose_beta_h_is_infinity(cc, valid):
    """on a handle of its own: the pair (-total_w, beta_h) is dropped, and what is left accepts total_c = O alone"""
    K = RV.key(4)
    rng = random.Random(204)
    gpu, slot = load(cc, K, beta_h_inf=True)
    try:
        good, bad = V.total_w_zero_rows(K, rng)
        rows = [valid[0][0], V.all_infinity_row(), good, bad, valid[0][1]]
        wants = check(cc, gpu, slot, K, rows, beta_h_inf=True)
        assert [w[0] for w in wants] == [REJECT, ACCEPT, ACCEPT, REJECT, REJECT]
    finally:
        gpu.close()


def test_a_batch_that_spans_two_chunks(cc, vk4, valid):
    """CHUNK + 5 showings tiled from five kinds: the second chunk starts at the right rows of every array"""
    K, gpu, slot = vk4
    x = valid[0][12]
    kinds = [valid[0][13], x.with_item("evals", 1, x.evals[1] ^ 1), valid[0][14], x.but(rho=1), V.forged_row(K, random.Random(205))]
    wants = check(cc, gpu, slot, K, kinds)
    assert [w[0] for w in wants] == [ACCEPT, REJECT, ACCEPT, MALFORMED, ACCEPT]
    n = CHUNK + 5
    a = [np.tile(np.frombuffer(b, np.uint8).reshape(5, -1), (n // 5 + 1, 1))[:n] for b in V.pack(kinds)]
    verdicts, k = cc.Groth16.range_verify_batch_packed(gpu, slot, *a)
    assert verdicts.shape == (n,) and k.shape == (n, 2, 32)
    for i in range(5):
        assert (verdicts[i::5] == wants[i][0]).all(), i
        assert (k[i::5].reshape(-1, 64) == np.frombuffer(wants[i][1], np.uint8)).all(), i


@pytest.mark.parametrize("n_bits", [2, 32])
def test_other_domain_sizes(cc, n_bits):
    K = RV.key(n_bits)
    rng = random.Random(206 + n_bits)
    gpu, slot = load(cc, K)
    try:
        rows = [V.valid_row(K, V.bases_of(), rng)[0], V.identity_breaker(K, rng), V.forged_row(K, rng)]
        assert V.pairing_by_trapdoor(K, *V.totals(K, n_bits, rows[1], V.parse(rows[1]))) and not V.identity_holds(n_bits, rows[1])
        wants = check(cc, gpu, slot, K, rows)
        assert [w[0] for w in wants] == [ACCEPT, REJECT, ACCEPT]
    finally:
        gpu.close()


def test_two_slots_on_one_handle(cc, vk4, valid):
    K, gpu, slot = vk4
    other = V.bases_of(V.B0 + 1, V.B1 + 1)
    slot2 = gpu.add_bases(*[unc(P) for P in other])
    assert slot2 != slot
    rows = valid[0][15:17]
    a = check(cc, gpu, slot, K, rows)
    b = check(cc, gpu, slot2, K, rows, bases=other)
    for (va, ka), (vb, kb) in zip(a, b):
        assert va == vb == ACCEPT and ka[:32] != kb[:32] and ka[32:] == kb[32:]      # k_0 follows the slot; the verdict and k_1 do not


def test_without_a_dleq_k_out_and_the_dleq_arrays_are_not_touched(cc, vk4, valid):
    K, gpu, slot = vk4
    x = valid[0][17]
    rows = [x, x.with_item("s", 5, x.s[5] ^ 1), x.with_item("evals", 0, x.evals[0] ^ 1), x.but(pok_c=R), x.but(rho=R)]
    verdicts, k = run(cc, gpu, slot, rows, pok=False)
    assert k is None
    assert list(verdicts) == [want(K, V.bases_of(), r, pok=False)[0] for r in rows] == [ACCEPT, ACCEPT, REJECT, ACCEPT, MALFORMED]
    a = [np.frombuffer(b, np.uint8).copy() for b in V.pack(rows)]
    out, k_out = np.zeros(5, np.uint8), np.full(5 * 64, 0xAB, np.uint8)
    p = lambda v: v.ctypes.data
    rc = cc.lib().cg_range_verify_batch(gpu._h, slot, None, p(a[1]), p(a[2]), p(a[3]), p(a[4]), p(a[5]), p(a[6]), p(a[7]), p(a[8]), None, None,
                                        5, p(out), p(k_out))
    assert rc == 0 and list(out) == list(verdicts) and (k_out == 0xAB).all()


def test_round_trip_with_show_range_batch(cc, vk4):
    K, gpu, slot = vk4
    rng = random.Random(207)
    bases = V.bases_of()
    openings = [(rng.randrange(16), rng.randrange(R)) for _ in range(3)]
    table = {}

    def challenge(phase, i, data):
        """a stand-in for Merlin: a function of the phase and the absorbed bytes alone"""
        data = np.asarray(data)
        assert data.shape == {"dleq": (4, 32), "c": (2, 32), "rho": (32,)}[phase]
        return table.setdefault((phase, data.tobytes()), rng.randrange(R))

    with cc.RangeProofKey(K.data, 4) as pk:
        proofs = cc.Groth16.show_range_batch(pk, pk.add_bases(*[unc(P) for P in bases]), openings, challenge)
    made = len(table)
    peds = [unc(RV.msm(bases, [m, r])) for m, r in openings]
    assert cc.Groth16.verify_range_batch(gpu, slot, peds, proofs, challenge) == [True] * 3
    assert len(table) == made                                       # the verifier absorbed exactly the bytes the prover did
    other = [unc(RV.msm(bases, [m ^ 1, r])) for m, r in openings]
    assert cc.Groth16.verify_range_batch(gpu, slot, other, proofs, challenge) == [False] * 3     # through the challenge comparison
    assert len(table) == made + 3
    assert cc.Groth16.verify_range_batch(gpu, slot, peds[:1] + other[1:2] + peds[2:], proofs, challenge, [(1, 2), (3, 4), (0, 0)]) == [True, False, True]
    assert cc.Groth16.verify_range_batch(gpu, slot, [], [], challenge) == []


def test_the_slot_limit_and_the_last_slot(cc, vk4, valid):
    """A key takes 64 slots (csrc/key_handle.hpp, PedersenSlots::MAX_SLOTS): the 65th registration is an argument error, and
    a proof verified on slot 63 gets the verdict and the k bytes slot 0 gives when both hold the same bases."""
    K = vk4[0]
    pair = [unc(P) for P in V.bases_of()]
    gpu, slot = load(cc, K)
    try:
        assert slot == 0 and [gpu.add_bases(*pair) for _ in range(63)] == list(range(1, 64))
        with pytest.raises(cc.CrescentGpuError, match="slots of this key are taken") as e:
            gpu.add_bases(*pair)
        assert e.value.code == INVALID_ARGUMENT
        rows = valid[0][18:19]
        (w_v, w_k), = check(cc, gpu, 0, K, rows)
        verdicts, k = run(cc, gpu, 63, rows)
        assert w_v == ACCEPT and verdicts[0] == w_v and k[0].tobytes() == w_k
    finally:
        gpu.close()


def test_argument_errors_under_a_handle(cc, vk4):
    K, gpu, slot = vk4
    L = cc.lib()
    buf = (ctypes.c_uint8 * 4096)()
    h = gpu._h
    full = [h, slot] + [buf] * 11 + [1, buf, buf]
    assert L.cg_range_verify_batch(*(full[:1] + [63] + full[2:])) == INVALID_ARGUMENT                    # a slot nobody registered
    assert b"slot 63" in L.cg_last_error()
    full0 = list(full)
    full0[13] = 0
    assert L.cg_range_verify_batch(*(full0[:1] + [63] + full0[2:])) == INVALID_ARGUMENT
    for i in (2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 15):             # every array but pok_c, whose absence has a meaning
        args = list(full)
        args[i] = None
        assert L.cg_range_verify_batch(*args) == INVALID_ARGUMENT, i
        assert b"null" in L.cg_last_error()
    assert L.cg_range_verify_batch(h, slot, *([None] * 11), 0, None, None) == 0                          # n = 0
    s = ctypes.c_uint32()
    good = b"".join(unc(P) for P in V.bases_of())
    off_curve = bytearray(good)
    off_curve[64] ^= 1
    assert L.cg_range_vk_add_bases(h, bytes(off_curve), ctypes.byref(s)) == INVALID_ARGUMENT
    assert L.cg_range_vk_add_bases(h, RV.fe(Q) + good[32:], ctypes.byref(s)) == INVALID_ARGUMENT
    group_ms, pairing_ms = gpu.last_kernel_ms()
    assert group_ms >= 0 and pairing_ms >= 0
