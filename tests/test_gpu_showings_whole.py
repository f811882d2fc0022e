"""Whole showings on the GPU (csrc/verify.hip: cg_verify_showings_batch, cg_show_shift_batch; csrc/show_link.hpp): the
cryptographic checks of `verify_show` (creds/src/lib.rs:630-658, :832-890) in one call - `ShowGroth16::verify` with its Merlin
transcript, per range proof the link ped_com = committed - t gamma_abc_g1[pos], and `ShowRange::verify` about that point.

Showings are made by the library (show_batch, show_shift_batch, range_prove_batch); what they are worth is judged by a
Python restatement of the three steps that reads their BYTES and shares no code with the library: ark's checked
deserialisation, the pairing of oracle/ark_files.py, the trapdoor verifier of tests/range_verify_vectors.py and the
pure-Python Merlin of tests/merlin_vectors.py.  Two layouts: [COMMITTED, REVEALED, HIDDEN] with one range, and an mDL-like
[COMMITTED, HIDDEN, COMMITTED, REVEALED] with two ranges on two slots and different shifts."""
import random
from dataclasses import dataclass, replace
from typing import List

import numpy as np
import pytest

import ark_files
import bn254_oracle as o
import merlin_vectors as MV
import range_vectors as RV
import range_verify_vectors as RVV
import show_vectors as S
import verify_vectors as V

pytestmark = pytest.mark.gpu

R, Q = o.R, o.Q
G1, F2 = o.G1, o.Fq2Ops
REJECT, ACCEPT, MALFORMED = 0, 1, 2
MADE, NOT_MADE = 1, 2
INVALID_ARGUMENT, MALFORMED_KEY = -1, -6
COM, HID, REV = S.COMMITTED, S.HIDDEN, S.REVEALED
LAYOUTS = {"one": [COM, REV, HID], "mdl": [COM, HID, COM, REV]}
CONTEXT = b"presentation message of a relying party"
VCHUNK = 1 << 15                             # showings per launch set (csrc/verify.hip, csrc/rangeverify.hip)
unc, cmp = o.g1_uncompressed, o.g1_compressed
fe, fes = RV.fe, RV.fes
val = lambda a: int.from_bytes(bytes(a), "little")


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


# ---- reading bytes as ark's checked deserialisation reads them -----------------------------------------------------------------
def compress_bytes(b) -> bytes:
    """an uncompressed G1 point's compressed form by arithmetic on its bytes alone, as the transcripts absorb it"""
    b = bytes(b)
    if b[63] & 0x40:
        return bytes(31) + b"\x40"
    y = int.from_bytes(b[32:63] + bytes([b[63] & 0x3F]), "little")
    return b[:31] + bytes([b[31] | (0x80 if y and y > Q - y else 0)])


def rd_g2_checked(b):
    """(ok, point or None): flags, coordinates < q, the twist equation, the r-torsion"""
    b = bytes(b)
    flags = b[127] & 0xC0
    c = [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(3)] + [int.from_bytes(b[96:127] + bytes([b[127] & 0x3F]), "little")]
    if flags == 0xC0 or any(v >= Q for v in c):
        return False, None
    if flags == 0x40:
        return True, None
    P = ((c[0], c[1]), (c[2], c[3]))
    if F2.sqr(P[1]) != F2.add(F2.mul(F2.sqr(P[0]), P[0]), o.B2):
        return False, None
    return o.G2.to_affine(o.G2.mul_affine(P, R)) is None, P


# ---- one showing as the call takes it ------------------------------------------------------------------------------------------
@dataclass
class Rec:
    revealed: List[int]
    rand_proof: bytes
    com_hidden: bytes
    committed: List[bytes]
    pok_c: int
    pok_s: List[int]              # flat, statement-major
    shifts: List[int]             # per link
    ranges: list                  # per link: (cc.RangeProof, (r_1, r_2))

    def but(self, **kw):
        return replace(self, **kw)


def range_rows(recs, j):
    ps = [x.ranges[j][0] for x in recs]
    cat = lambda f: b"".join(f(p) for p in ps)
    return (cat(lambda p: bytes(p.com_f)), cat(lambda p: bytes(p.com_g)), cat(lambda p: bytes(p.com_q)),
            cat(lambda p: fe(p.eval_g) + fe(p.eval_gw) + fe(p.eval_w_hat)), cat(lambda p: bytes(p.proof_g) + bytes(p.proof_gw) + bytes(p.proof_w_hat)),
            b"".join(r.to_bytes(16, "little") for x in recs for r in x.ranges[j][1]), cat(lambda p: fe(p.dleq_c)),
            cat(lambda p: fes(s for si in p.dleq_s for s in si)))


def show_arrays(recs):
    """revealed, rand_proofs, com_hidden, committed, pok_c, pok_s"""
    j = lambda f: b"".join(f(x) for x in recs)
    return (j(lambda x: fes(x.revealed)), j(lambda x: x.rand_proof), j(lambda x: x.com_hidden), j(lambda x: b"".join(x.committed)),
            j(lambda x: fe(x.pok_c)), j(lambda x: fes(x.pok_s)))


class World:
    """one Groth16 key from chosen scalars (gamma = 1) under a layout, one range key with a slot per committed input on the
    proving and on the verifying side, and the oracles' view of both"""

    def __init__(self, cc, layout, n_bits, seed):
        self.cc, self.io, self.n_bits = cc, LAYOUTS[layout], n_bits
        self.rng, self.sc = V.synthetic_scalars(len(self.io), seed, gamma=1)
        self.vk = V.synthetic_vk(*self.sc[:4], self.sc[4])
        self.com = [i for i, t in enumerate(self.io) if t == COM]
        self.hid = [i for i, t in enumerate(self.io) if t == HID]
        self.n_rand = cc.show_rand_count(self.io)
        self.pvk = cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(self.vk)))
        self.K = RV.key(n_bits)
        self.rpk = cc.RangeProofKey(self.K.data, n_bits)
        self.rvk = cc.RangeVerifyingKey(RVV.vk_bytes(self.K), n_bits)
        gabc, delta = self.vk["gamma_abc_g1"], self.vk["delta_g1"]
        self.bases = [[gabc[i + 1], delta] for i in self.com]
        self.pslots = [self.rpk.add_bases(unc(b[0]), unc(b[1])) for b in self.bases]
        self.vslots = [self.rvk.add_bases(unc(b[0]), unc(b[1])) for b in self.bases]
        self.links = [(ci, self.vslots[ci]) for ci in range(len(self.com))]
        self.ora = ark_files.prepare_verifying_key(self.vk)
        self.cfb = [cmp(P) for P in self.K.pgam[:3] + [self.K.pg[0]]]
        self._pairing, self._range = {}, {}

    def close(self):
        for h in (self.pvk, self.rpk, self.rvk):
            h.close()

    # -- making showings with the library ---------------------------------------------------------------------------------------
    def inputs(self, shifts, ms):
        """public inputs whose committed ones are shift + m, m the value the range proof is about"""
        xs = [self.rng.randrange(R) for _ in self.io]
        for ci, i in enumerate(self.com):
            xs[i] = (shifts[ci] + ms[ci]) % R
        return xs

    def rand_rows(self, n):
        return [[self.rng.randrange(1, R), self.rng.randrange(1, R)] + [self.rng.randrange(R) for _ in range(self.n_rand - 2)] for _ in range(n)]

    def make(self, xs_list, shifts_list, rows, context=CONTEXT):
        """show_batch, then per link show_shift_batch and range_prove_batch: the creating side as INTEGRATION.md lays it out"""
        G, rng = self.cc.Groth16, self.rng
        n = len(xs_list)
        states = [(V.proof_bytes(V.synthetic_proof(self.sc, xs, a=rng.randrange(1, R), b=rng.randrange(1, R))), xs) for xs in xs_list]
        shows = G.show_batch(self.pvk, self.io, states, rand=rows, context=context)
        ranges = [[] for _ in range(n)]
        for j, (ci, _) in enumerate(self.links):
            openings = [(xs_list[i][self.com[ci]], rows[i][2 + ci]) for i in range(n)]
            out, ped, status = G.show_shift_batch(self.pvk, self.com[ci], openings, [shows[i].commited_inputs[ci] for i in range(n)],
                                                  [shifts_list[i][j] for i in range(n)])
            assert list(status) == [MADE] * n
            proofs = G.prove_range_batch(self.rpk, self.pslots[ci], [(val(out[i, 0]), val(out[i, 1])) for i in range(n)],
                                         [ped[i].tobytes() for i in range(n)], [[rng.randrange(R) for _ in range(RV.N_RAND)] for _ in range(n)])
            for i in range(n):
                ranges[i].append((proofs[i], (rng.getrandbits(128), rng.getrandbits(128))))
        return [Rec([x for x, t in zip(xs_list[i], self.io) if t == REV], bytes(sg.rand_proof), bytes(sg.com_hidden_inputs),
                    [bytes(c) for c in sg.commited_inputs], sg.pok_c, [s for si in sg.pok_s for s in si], list(shifts_list[i]), ranges[i])
                for i, sg in enumerate(shows)]

    # -- the call ---------------------------------------------------------------------------------------------------------------
    def verify(self, recs, context=CONTEXT, links=None, **kw):
        links = self.links if links is None else links
        shifts = b"".join(fes(x.shifts) for x in recs)
        return self.cc.Groth16.verify_showings_batch_packed(self.pvk, self.rvk, self.io, *show_arrays(recs), links, shifts,
                                                            [range_rows(recs, j) for j in range(len(links))], context, **kw)

    # -- the restatement of verify_show's three steps ------------------------------------------------------------------------------
    def groth_part(self, x: Rec, context):
        """`ShowGroth16::verify` on the showing's bytes: the pairing and the transcript's challenge against pok_c"""
        key = (x.rand_proof, x.com_hidden, tuple(x.committed), tuple(x.revealed), x.pok_c, tuple(x.pok_s))
        if key not in self._pairing:
            ok_a, A = RVV.rd_g1_checked(x.rand_proof[:64])
            ok_b, B = rd_g2_checked(x.rand_proof[64:192])
            ok_c, C = RVV.rd_g1_checked(x.rand_proof[192:])
            ok_h, comh = RVV.rd_g1_checked(x.com_hidden)
            coms = [RVV.rd_g1_checked(b) for b in x.committed]
            ok = ok_a and ok_b and ok_c and ok_h and all(g for g, _ in coms) and all(v < R for v in x.revealed + [x.pok_c] + x.pok_s)
            if not ok:
                self._pairing[key] = (MALFORMED, None)
            else:
                s, at = [], 0
                for k in [2] * len(self.com) + [len(self.hid) + 1]:
                    s.append(x.pok_s[at:at + k])
                    at += k
                sh = S.Show((A, B, C), comh, [P for _, P in coms], x.pok_c, s, list(x.revealed))
                verdict = ACCEPT if S.accepts(self.ora, self.vk, self.io, sh) else REJECT
                st = [([cmp(b) for b in bases], cmp(k), compress_bytes(y)) for bases, k, y in
                      zip(S.verifier_bases(self.vk, self.io), S.recomputed_k(self.vk, self.io, sh), x.committed + [x.com_hidden])]
                self._pairing[key] = (verdict, st)
        verdict, st = self._pairing[key]
        if verdict != ACCEPT:
            return verdict
        return ACCEPT if MV.to_int(MV.dlog_challenge(context, st)) == x.pok_c else REJECT

    def ped_com(self, x: Rec, link, j):
        """the link on bytes: (ok, committed[ci] - t gamma_abc_g1[pos]), affine or None"""
        ci, t = link[0], x.shifts[j]
        ok, P = RVV.rd_g1_checked(x.committed[ci])
        if not ok or t >= R:
            return False, None
        if t == 0:
            return True, P
        minus = G1.mul_affine(self.bases[ci][0], (-t) % R)
        return True, G1.to_affine(minus if P is None else G1.add_affine(minus, P))

    def range_part(self, x: Rec, link, j):
        """the link, then `ShowRange::verify` about it: the trapdoor verifier and the DLEQ's transcript"""
        p, (r1, r2) = x.ranges[j]
        key = (x.committed[link[0]], x.shifts[j], link[0], p.to_bytes(), r1, r2)
        if key not in self._range:
            ok, ped = self.ped_com(x, link, j)
            if not ok:
                self._range[key] = MALFORMED
            else:
                c, rho = MV.range_challenges(compress_bytes(p.com_f), compress_bytes(p.com_g), compress_bytes(p.com_q))
                pr = [bytes(b) for b in (p.proof_g, p.proof_gw, p.proof_w_hat)]
                row = RVV.Row(unc(ped), bytes(p.com_f), bytes(p.com_g), bytes(p.com_q), [p.eval_g, p.eval_gw, p.eval_w_hat], [b[:64] for b in pr],
                              [val(b[64:]) for b in pr], MV.to_int(c), MV.to_int(rho), r1, r2, p.dleq_c, [s for si in p.dleq_s for s in si])
                bases = self.bases[link[0]]
                verdict, kb = RVV.expected(self.K, bases, row)
                if verdict == ACCEPT:
                    cd = MV.range_dleq_challenge([cmp(B) for B in bases], self.cfb, kb[:32], kb[32:], cmp(ped), compress_bytes(p.com_f))
                    if MV.to_int(cd) != p.dleq_c:
                        verdict = REJECT
                self._range[key] = verdict
        return self._range[key]

    def want(self, recs, context=CONTEXT, links=None):
        """(verdicts, part verdicts) as lists"""
        links = self.links if links is None else links
        parts = [[self.groth_part(x, context)] + [self.range_part(x, link, j) for j, link in enumerate(links)] for x in recs]
        return [MALFORMED if MALFORMED in p else ACCEPT if all(v == ACCEPT for v in p) else REJECT for p in parts], parts


def check(w, recs, **kw):
    """the call against the restatement, every byte; returns the parts"""
    verdicts, parts = w.verify(recs, **kw)
    want_v, want_p = w.want(recs, **kw)
    assert parts.tolist() == want_p
    assert verdicts.tolist() == want_v
    return want_v, want_p


_worlds = {}


@pytest.fixture(scope="module")
def worlds(cc):
    def get(layout, n_bits=4):
        if (layout, n_bits) not in _worlds:
            _worlds[layout, n_bits] = World(cc, layout, n_bits, 0x5803 + n_bits + len(layout))
        return _worlds[layout, n_bits]
    yield get
    for w in _worlds.values():
        w.close()
    _worlds.clear()


@pytest.fixture(scope="module")
def six(worlds):
    """six showings under the mDL-like layout, made once and left as they are.  3 has small shifts, so that its committed
    values are themselves in range; 4 has commitment randomness 0 on its first input and that input as the shift, which makes
    ped_com = O"""
    w = worlds("mdl")
    rng = w.rng
    shifts = [[rng.randrange(1, 1 << 40), rng.randrange(1, 1 << 20)] for _ in range(6)]
    ms = [[rng.randrange(1 << 4), rng.randrange(1 << 4)] for _ in range(6)]
    shifts[3], ms[3] = [3, 2], [5, 9]
    ms[4][0] = 0
    rows = w.rand_rows(6)
    rows[4][2] = 0
    xs = [w.inputs(t, m) for t, m in zip(shifts, ms)]
    recs = w.make(xs, shifts, rows)
    return w, recs, xs, rows


# ---- 1. the round trip -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,n_bits,n", [("one", 4, 1), ("mdl", 4, 3), ("one", 8, 65), ("mdl", 4, 65)])
def test_round_trip(cc, worlds, layout, n_bits, n):
    """show_batch, show_shift_batch, range_prove_batch, verify_showings_batch: a lone showing, an odd count, one past a
    64-lane workgroup; n_bits = 8 once"""
    w = worlds(layout, n_bits)
    rng = w.rng
    base = []
    for _ in range(min(n, 3)):                # client states are tiled, the randomness of every showing is its own
        shifts = [rng.randrange(1 << 62) for _ in w.com]
        base.append((shifts, w.inputs(shifts, [rng.randrange(1 << n_bits) for _ in w.com])))
    shifts = [base[i % len(base)][0] for i in range(n)]
    recs = w.make([base[i % len(base)][1] for i in range(n)], shifts, w.rand_rows(n))
    verdicts, parts = w.verify(recs)
    assert verdicts.tolist() == [ACCEPT] * n
    assert parts.tolist() == [[ACCEPT] * (1 + len(w.com))] * n
    assert w.want(recs[:2]) == ([ACCEPT] * len(recs[:2]), [[ACCEPT] * (1 + len(w.com))] * len(recs[:2]))
    # the same through the classes
    G = cc.Groth16
    shows = [(cc.ShowGroth16(x.rand_proof, x.com_hidden, x.pok_c, _nested(w, x.pok_s), x.committed), x.revealed) for x in recs]
    got = G.verify_showings_batch(w.pvk, w.rvk, w.io, shows, w.links, [x.shifts for x in recs], [[p for p, _ in x.ranges] for x in recs], CONTEXT)
    assert got == [True] * n
    # n_ranges = 0 is ShowGroth16::verify whole, with no range key at all
    v0, p0 = G.verify_showings_batch_packed(w.pvk, None, w.io, *show_arrays(recs), [], b"", [], CONTEXT)
    assert v0.tolist() == [ACCEPT] * n and p0.tolist() == [[ACCEPT]] * n
    assert G.verify_showings_batch(w.pvk, None, w.io, shows, [], [[]] * n, [[]] * n, b"another context") == [False] * n


def _nested(w, flat):
    out, at = [], 0
    for k in [2] * len(w.com) + [len(w.hid) + 1]:
        out.append(list(flat[at:at + k]))
        at += k
    return out


# ---- 3. the link ------------------------------------------------------------------------------------------------------------------
def link_faults(w, recs, xs, rows):
    """one fault per showing among valid ones: 1 a shift of t + 1, 3 a range proof made for the unshifted commitment"""
    G = w.cc.Groth16
    bad = list(recs)
    bad[1] = recs[1].but(shifts=[recs[1].shifts[0] + 1, recs[1].shifts[1]])
    ci = 1
    opening = (xs[3][w.com[ci]], rows[3][2 + ci])
    assert opening[0] < 1 << w.n_bits
    unshifted = G.prove_range_batch(w.rpk, w.pslots[ci], [opening], [recs[3].committed[ci]], [[w.rng.randrange(R) for _ in range(RV.N_RAND)]])[0]
    bad[3] = recs[3].but(ranges=[recs[3].ranges[0], (unshifted, recs[3].ranges[1][1])])
    return bad


def test_link_faults(six):
    w, recs, xs, rows = six
    verdicts, parts = check(w, recs)
    assert verdicts == [ACCEPT] * 6 and parts == [[ACCEPT] * 3] * 6
    ok, ped = w.ped_com(recs[4], w.links[0], 0)
    assert ok and ped is None                                      # ped_com = O is legal, and the oracle accepts it
    bad = link_faults(w, recs, xs, rows)
    verdicts, parts = check(w, bad)
    assert verdicts == [ACCEPT, REJECT, ACCEPT, REJECT, ACCEPT, ACCEPT]
    assert parts[1] == [ACCEPT, REJECT, ACCEPT] and parts[3] == [ACCEPT, ACCEPT, REJECT]
    # the unshifted proof is a good one about the committed point itself: with a zero shift it verifies
    assert check(w, [bad[3].but(shifts=[bad[3].shifts[0], 0])])[1] == [[ACCEPT] * 3]
    # the two links swapped: each range proof is checked against the other committed input, under that input's slot
    swapped = [w.links[1], w.links[0]]
    verdicts, parts = check(w, recs, links=swapped)
    assert verdicts == [REJECT] * 6 and all(p[0] == ACCEPT and ACCEPT not in p[1:] for p in parts)
    # a shift that makes ped_com = O under a proof about another point, and a zero shift under a proof about the shifted one
    at_o = recs[4].but(ranges=[recs[2].ranges[0], recs[4].ranges[1]])
    moved = recs[0].but(shifts=[0, recs[0].shifts[1]])
    verdicts, parts = check(w, [recs[2], at_o, moved, recs[5]])
    assert verdicts == [ACCEPT, REJECT, REJECT, ACCEPT] and parts[1] == [ACCEPT, REJECT, ACCEPT] and parts[2] == [ACCEPT, REJECT, ACCEPT]


# ---- 2. agreement with the separate calls --------------------------------------------------------------------------------------
def test_parts_equal_the_separate_calls(six):
    w, recs, xs, rows = six
    G = w.cc.Groth16
    bad = link_faults(w, recs, xs, rows)
    bad[5] = bad[5].but(pok_c=bad[5].pok_c ^ 1)
    _, parts = w.verify(bad)
    arrays = show_arrays(bad)
    verdicts, k = G.verify_show_batch_packed(w.pvk, w.io, *arrays)
    cs = G.show_dlog_challenges(w.pvk, w.io, k, np.frombuffer(arrays[3], np.uint8), np.frombuffer(arrays[2], np.uint8), CONTEXT)
    groth = [ACCEPT if v == ACCEPT and cs[i].tobytes() == fe(bad[i].pok_c) else REJECT if v == ACCEPT else int(v) for i, v in enumerate(verdicts)]
    assert parts[:, 0].tolist() == groth and groth[5] == REJECT
    for j, link in enumerate(w.links):
        peds = b"".join(unc(w.ped_com(x, link, j)[1]) for x in bad)
        f, g, q, ev, pr, rz, pc, ps = range_rows(bad, j)
        alone = G.range_verify_proofs_batch_packed(w.rvk, link[1], peds, f, g, q, ev, pr, rz, pc, ps)
        assert parts[:, 1 + j].tolist() == alone.tolist(), j


# ---- 4. the challenge ----------------------------------------------------------------------------------------------------------------
def test_challenge(six):
    w, recs, _, _ = six
    other = bytearray(CONTEXT)
    other[7] ^= 1
    verdicts, parts = check(w, recs, context=bytes(other))
    assert verdicts == [REJECT] * 6 and parts == [[REJECT, ACCEPT, ACCEPT]] * 6
    assert check(w, recs, context=None)[0] == [REJECT] * 6
    bad = list(recs)
    bad[2] = recs[2].but(pok_c=recs[2].pok_c ^ (1 << 100))
    verdicts, parts = check(w, bad)
    assert verdicts == [ACCEPT, ACCEPT, REJECT, ACCEPT, ACCEPT, ACCEPT] and parts[2] == [REJECT, ACCEPT, ACCEPT]
    # one context per showing, strided: only the showing whose own context is the right one stays
    stride = len(CONTEXT) + 5
    ctx = b"".join((CONTEXT if i == 4 else bytes(other)) + bytes(5) for i in range(6))[:-5]
    verdicts, _ = w.verify(recs, context=ctx, context_len=len(CONTEXT), context_stride=stride)
    assert verdicts.tolist() == [REJECT] * 4 + [ACCEPT, REJECT]


# ---- 5. malformed inputs ---------------------------------------------------------------------------------------------------------------
def malformed_batch(w, recs):
    bad = list(recs)
    bad[0] = recs[0].but(shifts=[R, recs[0].shifts[1]])                               # a shift >= r
    p, rz = recs[1].ranges[1]
    off = bytearray(p.com_q)
    off[0] ^= 1
    assert not RVV.rd_g1_checked(bytes(off))[0]
    bad[1] = recs[1].but(ranges=[recs[1].ranges[0], (replace(p, com_q=bytes(off)), rz)])     # com_q off the curve
    off = bytearray(recs[2].committed[0])
    off[0] ^= 1
    assert not RVV.rd_g1_checked(bytes(off))[0]
    bad[2] = recs[2].but(committed=[bytes(off), recs[2].committed[1]])                # a committed point off the curve
    outside = o.g2_uncompressed(V.twist_point_outside_g2(random.Random(9)))
    bad[4] = recs[4].but(rand_proof=recs[4].rand_proof[:64] + outside + recs[4].rand_proof[192:])       # B outside the r-torsion
    return bad


def test_malformed_inputs(six):
    w, recs, _, _ = six
    verdicts, parts = check(w, malformed_batch(w, recs))
    assert verdicts == [MALFORMED, MALFORMED, MALFORMED, ACCEPT, MALFORMED, ACCEPT]
    assert parts[0] == [ACCEPT, MALFORMED, ACCEPT] and parts[1] == [ACCEPT, ACCEPT, MALFORMED]
    assert parts[2] == [MALFORMED, MALFORMED, ACCEPT] and parts[4] == [MALFORMED, ACCEPT, ACCEPT]


# ---- 6. argument errors ---------------------------------------------------------------------------------------------------------------
def test_argument_errors(cc, six, worlds):
    w, recs, _, _ = six
    L = cc.lib()
    from crescent_credentials_amd import api
    n = len(recs)
    keep = [np.frombuffer(a, np.uint8).copy() for a in show_arrays(recs)]
    rows = [[np.frombuffer(a, np.uint8).copy() for a in range_rows(recs, j)] for j in range(2)]
    shifts = np.frombuffer(b"".join(fes(x.shifts) for x in recs), np.uint8).copy()
    io = np.array(w.io, np.uint8)
    ctx = np.frombuffer(CONTEXT, np.uint8).copy()
    verdicts, parts = np.full(n, 7, np.uint8), np.full((n, 3), 7, np.uint8)
    ptr = lambda a: a.ctypes.data
    links_of = lambda pairs: (api._CgShowRangeLink * 2)(*[api._CgShowRangeLink(a, b) for a, b in pairs])
    rows_of = lambda rs: (api._CgRangeRows * 2)(*[api._CgRangeRows(*[None if a is None else ptr(a) for a in r]) for r in rs])

    def call(pvk=w.pvk, rvk=w.rvk, io=io, n_io=len(w.io), arrays=keep, links=w.links, shifts=shifts, rows=rows, n=n, verdicts=verdicts):
        return L.cg_verify_showings_batch(pvk._h, rvk._h, ptr(io), n_io, ptr(ctx), ctx.size, 0, *[None if a is None else ptr(a) for a in arrays], 2,
                                          None if links is None else links_of(links), None if shifts is None else ptr(shifts),
                                          None if rows is None else rows_of(rows), n, None if verdicts is None else ptr(verdicts), ptr(parts))

    assert call() == 0 and verdicts.tolist() == [ACCEPT] * n
    verdicts[:], parts[:] = 7, 7
    # a slot whose bases belong to another input; an unknown slot; committed_index out of range
    assert call(links=[(0, w.vslots[1]), (1, w.vslots[1])]) == INVALID_ARGUMENT and b"gamma_abc_g1" in L.cg_last_error()
    assert call(links=[(0, w.vslots[0]), (1, 63)]) == INVALID_ARGUMENT
    assert call(links=[(0, w.vslots[0]), (2, w.vslots[1])]) == INVALID_ARGUMENT and b"committed_index" in L.cg_last_error()
    # null arrays
    for i in range(len(keep)):
        assert call(arrays=[None if k == i else a for k, a in enumerate(keep)]) == INVALID_ARGUMENT, i
    for i in range(8):
        assert call(rows=[rows[0], [None if k == i else a for k, a in enumerate(rows[1])]]) == INVALID_ARGUMENT, i
    assert call(links=None) == INVALID_ARGUMENT and call(shifts=None) == INVALID_ARGUMENT and call(rows=None) == INVALID_ARGUMENT
    assert call(verdicts=None) == INVALID_ARGUMENT
    class Null:
        _h = None
    assert call(pvk=Null) == INVALID_ARGUMENT and call(rvk=Null) == INVALID_ARGUMENT
    # a wrong n_io, and a byte that is no PublicIOType
    assert call(n_io=len(w.io) - 1) == MALFORMED_KEY
    assert call(io=np.array(w.io[:-1] + [3], np.uint8)) == INVALID_ARGUMENT
    # a range key whose slot was registered for another Groth16 key's bases
    other = worlds("one")
    assert call(rvk=other.rvk) == INVALID_ARGUMENT
    assert (verdicts == 7).all() and (parts == 7).all()                # no error touched an output
    assert call(n=0) == 0 and (verdicts == 7).all()
    assert L.cg_pvk_set_showings_overlap(w.pvk._h, 2) == INVALID_ARGUMENT and L.cg_pvk_set_showings_overlap(None, 1) == INVALID_ARGUMENT
    # cg_show_shift_batch
    buf = np.zeros(64, np.uint8)
    assert L.cg_show_shift_batch(w.pvk._h, len(w.io), ptr(buf), ptr(buf), ptr(buf), 1, ptr(buf), ptr(buf), ptr(buf)) == INVALID_ARGUMENT
    for i in range(6):
        args = [None if k == i else ptr(buf) for k in range(6)]
        assert L.cg_show_shift_batch(w.pvk._h, 0, *args[:3], 1, *args[3:]) == INVALID_ARGUMENT, i
    assert L.cg_show_shift_batch(w.pvk._h, 0, None, None, None, 0, None, None, None) == 0
    assert L.cg_show_shift_batch(None, 0, ptr(buf), ptr(buf), ptr(buf), 1, ptr(buf), ptr(buf), ptr(buf)) == INVALID_ARGUMENT


# ---- 7. latency mode, and the two orders of the halves -------------------------------------------------------------------------------
def test_latency_mode_and_order_give_the_same_bytes(six):
    w, recs, xs, rows = six
    batch = link_faults(w, recs, xs, rows) + malformed_batch(w, recs)
    wide = [a.tobytes() for a in w.verify(batch)]
    try:
        for lat_pvk, lat_rvk in ((True, False), (False, True), (True, True)):
            w.pvk.set_latency(lat_pvk)
            w.rvk.set_latency(lat_rvk)
            assert [a.tobytes() for a in w.verify(batch)] == wide, (lat_pvk, lat_rvk)
        for lat in (False, True):
            w.pvk.set_latency(lat)
            w.rvk.set_latency(lat)
            w.pvk.set_showings_overlap(False)
            assert [a.tobytes() for a in w.verify(batch)] == wide, lat
            w.pvk.set_showings_overlap(True)
    finally:
        w.pvk.set_latency(False)
        w.rvk.set_latency(False)
        w.pvk.set_showings_overlap(True)


# ---- 8. the chunk edge -----------------------------------------------------------------------------------------------------------------
def test_one_past_a_chunk(worlds):
    """one valid and one link-faulted showing tiled to VCHUNK + 1: the verdicts follow the tiling, across the chunk edge of
    both handles' buffers"""
    w = worlds("one")
    rng = w.rng
    shifts = [[rng.randrange(1 << 62)] for _ in range(2)]
    xs = [w.inputs(t, [rng.randrange(1 << 4)]) for t in shifts]
    pair = w.make(xs, shifts, w.rand_rows(2))
    pair[1] = pair[1].but(shifts=[pair[1].shifts[0] + 1])
    _, want = check(w, pair)
    assert want == [[ACCEPT, ACCEPT], [ACCEPT, REJECT]]
    n = VCHUNK + 1
    idx = np.arange(n) % 2
    tile = lambda b: np.frombuffer(b, np.uint8).reshape(2, -1)[idx].copy()
    verdicts, parts = w.cc.Groth16.verify_showings_batch_packed(
        w.pvk, w.rvk, w.io, *[tile(a) for a in show_arrays(pair)], w.links, tile(b"".join(fes(x.shifts) for x in pair)),
        [tuple(tile(a) for a in range_rows(pair, 0))], CONTEXT)
    assert (verdicts == np.array([ACCEPT, REJECT], np.uint8)[idx]).all()
    assert (parts == np.array(want, np.uint8)[idx]).all()
    assert verdicts[VCHUNK - 1] == REJECT and verdicts[VCHUNK] == ACCEPT


# ---- 9. show_shift_batch -----------------------------------------------------------------------------------------------------------------
def test_show_shift_batch(worlds):
    w = worlds("mdl")
    G, rng = w.cc.Groth16, w.rng
    pos = w.com[1]
    base, delta = w.bases[1]
    b, d = w.sc[4][pos + 1], w.sc[3]                      # base = b G, delta_g1 = d G
    com = lambda m, r: RV.g1(m * b + r * d)
    t64 = rng.getrandbits(64)
    cases = [(rng.randrange(R), rng.randrange(R), rng.randrange(R)), (5, rng.randrange(R), 9),        # m < t: wraps mod r
             (t64 + 3, rng.randrange(R), t64), (t64, 0, t64),                                          # c = t base: ped_com = O
             (0, 0, 0), (7, rng.randrange(R), 0), (0, rng.randrange(R), R - 1)]
    points = [com(m, r) for m, r, _ in cases]
    points[4] = None                                                                                   # c = O, t = 0
    want_open = [fe((m - t) % R) + fe(r) for m, r, t in cases]
    want_ped = [unc(RV.g1(m * b + r * d - t * b)) for m, r, t in cases]
    assert want_ped[3] == unc(None) and want_ped[4] == unc(None)
    out, ped, status = G.show_shift_batch(w.pvk, pos, [(m, r) for m, r, _ in cases], [unc(P) for P in points], [t for _, _, t in cases])
    assert status.tolist() == [MADE] * len(cases)
    assert [out[i].tobytes() for i in range(len(cases))] == want_open
    assert [ped[i].tobytes() for i in range(len(cases))] == want_ped
    # a scalar >= r, or a commitment off the curve: that row only, zero bytes
    off = bytearray(unc(points[0]))
    off[0] ^= 1
    assert not RVV.rd_g1_checked(bytes(off))[0]
    m, r, t = cases[0]
    rows = [(R, r, t, unc(points[0])), (m, r, t, unc(points[0])), (m, R + 1, t, unc(points[0])), (m, r, R, unc(points[0])), (m, r, t, bytes(off)),
            cases[1] + (unc(points[1]),)]
    out, ped, status = G.show_shift_batch(w.pvk, pos, b"".join(fe(a) + fe(c) for a, c, _, _ in rows), [p for _, _, _, p in rows],
                                          b"".join(fe(c) for _, _, c, _ in rows))
    assert status.tolist() == [NOT_MADE, MADE, NOT_MADE, NOT_MADE, NOT_MADE, MADE]
    for i, made in enumerate(status.tolist()):
        if made == MADE:
            twin = 1 if i == 5 else 0
            assert out[i].tobytes() == want_open[twin] and ped[i].tobytes() == want_ped[twin], i
        else:
            assert not out[i].any() and not ped[i].any(), i
