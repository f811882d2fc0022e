"""Test vectors for showings (csrc/verify.hip, cg_verify_show_batch), built with the oracle only, exactly as the wallet
builds them: `rerandomize_proof` (forks/groth16/src/prover.rs:227-254) with chosen r1, r2, then `show_groth16`
(creds/src/groth16rand.rs:100-187) with chosen commitment randomness r_i and z, C' = C - (acc_r + z)·G.  That last step
is sound only for the fork's gamma = 1 keys (generator.rs:28): the golden keys are such keys, synthetic ones must set
gamma = 1.  The DLogPoK needs no real challenge: pick nonces rho_ij and any c < 2^248, set s_ij = rho_ij - c·x_ij; the
k_i a verifier recomputes (creds/src/dlog.rs:137-145) is then both msm(bases ‖ y_i, s ‖ c) and Σ rho_ij·base_ij, and
make_show asserts the two agree.  Shared by tests/test_show_cpu.py, tests/test_gpu_show.py and tools/probe_verify_show.py."""
import struct
from dataclasses import dataclass, field
from typing import List

import ark_files
import bn254_oracle as o

Q, R = o.Q, o.R
G1, G2 = o.G1, o.G2
REVEALED, HIDDEN, COMMITTED = 0, 1, 2


def _aff(J):
    return G1.to_affine(J)


def _mul(P, k):
    return G1.mul_affine(P, k % R)


def _msm(bases, scalars):
    return _aff(G1.msm_naive(bases, [s % R for s in scalars]))


def rerandomize(vk, proof, r1, r2):
    """prover.rs:239-253: A' = (1/r1)A, B' = r1 B + r1 r2 delta_g2, C' = C + r2 A"""
    a, b, c = proof
    assert r1 % R and r2 % R
    na = _aff(_mul(a, pow(r1, R - 2, R)))
    nb = G2.to_affine(G2.add(G2.mul_affine(b, r1 % R), G2.mul_affine(vk["delta_g2"], r1 * r2 % R)))
    nc = _aff(G1.add_affine(_mul(a, r2), c))
    return (na, nb, nc)


@dataclass
class Show:
    rand_proof: tuple                 # (A', B', C'') affine
    com_hidden: object                # affine G1 or None
    committed: list                   # affine G1 per committed input
    c: int
    s: List[List[int]]                # responses, statement-major
    revealed: List[int]               # the revealed inputs in input order
    bases: list = field(default_factory=list)     # per statement, as the verifier rebuilds them (groth16rand.rs:266-282)
    k: list = field(default_factory=list)         # the expected recomputed k_i, affine

    @property
    def y(self):
        return list(self.committed) + [self.com_hidden]


def make_show(vk, proof, inputs, io_types, rng, r1=None, r2=None, rs=None, z=None, c=None, rho=None) -> Show:
    """groth16rand.rs:100-187 with every random value chosen by the caller or drawn from rng.  rs: the committed inputs'
    randomness in order; rho: {statement index: nonces} overrides."""
    assert len(inputs) == len(io_types) == len(vk["gamma_abc_g1"]) - 1
    r1 = rng.randrange(1, R) if r1 is None else r1
    r2 = rng.randrange(1, R) if r2 is None else r2
    rand = rerandomize(vk, proof, r1, r2)
    gabc, delta = vk["gamma_abc_g1"], vk["delta_g1"]
    n_com = sum(1 for t in io_types if t == COMMITTED)
    rs = [rng.randrange(R) for _ in range(n_com)] if rs is None else list(rs)
    z = rng.randrange(R) if z is None else z
    y, bases, scalars = [], [], []
    hid_bases, hid_scalars = [], []
    acc_r, ci = 0, 0
    for i, t in enumerate(io_types):
        if t == HIDDEN:
            hid_bases.append(gabc[i + 1]); hid_scalars.append(inputs[i])
        elif t == COMMITTED:
            r = rs[ci]; ci += 1
            acc_r += r
            y.append(_msm([delta, gabc[i + 1]], [r, inputs[i]]))            # :133
            bases.append([gabc[i + 1], delta]); scalars.append([inputs[i], r])
    hid_scalars.append(z); hid_bases.append(delta)                          # :156-158
    com_hidden = _msm(hid_bases, hid_scalars)
    bases.append(hid_bases); scalars.append(hid_scalars); y.append(com_hidden)
    new_c = _aff(G1.add_affine(_mul(o.G1_GEN, -(acc_r + z)), rand[2]))      # :167-168
    # DLogPoK::prove (dlog.rs:60-109) without the transcript
    c = rng.randrange(1 << 248) if c is None else c
    s, k = [], []
    for i in range(len(y)):
        nonce = rho[i] if rho and i in rho else [rng.randrange(R) for _ in bases[i]]
        s.append([(n - c * x) % R for n, x in zip(nonce, scalars[i])])
        ki = _msm(bases[i], nonce)
        assert ki == _msm(bases[i] + [y[i]], s[i] + [c])                   # what dlog.rs:137-145 recomputes
        k.append(ki)
    return Show((rand[0], rand[1], new_c), com_hidden, y[:-1], c, s, [x for x, t in zip(inputs, io_types) if t == REVEALED], bases, k)


def verifier_bases(vk, io_types):
    """the bases `ShowGroth16::verify` hands to `DLogPoK::verify` (groth16rand.rs:258-282)"""
    gabc, delta = vk["gamma_abc_g1"], vk["delta_g1"]
    out = [[gabc[i + 1], delta] for i, t in enumerate(io_types) if t == COMMITTED]
    out.append([gabc[i + 1] for i, t in enumerate(io_types) if t == HIDDEN] + [delta])
    return out


def prepared_inputs(vk, io_types, sh: Show):
    """groth16rand.rs:246-279, affine"""
    gabc = vk["gamma_abc_g1"]
    acc = G1.add_affine(G1.to_jac(sh.com_hidden), gabc[0])
    for P in sh.committed:
        acc = G1.add_affine(acc, P)
    rev = [gabc[i + 1] for i, t in enumerate(io_types) if t == REVEALED]
    acc = G1.add(acc, G1.msm_naive(rev, [x % R for x in sh.revealed]))
    return _aff(acc)


def recomputed_k(vk, io_types, sh: Show):
    """dlog.rs:134-145 on the showing as it stands (tampered or not), affine"""
    return [_msm(b + [yi], si + [sh.c]) for b, yi, si in zip(verifier_bases(vk, io_types), sh.y, sh.s)]


def pairing_accepts(vk, io_types, sh: Show) -> bool:
    """verify_proof_with_prepared_inputs (verifier.rs:44-65) as one pairing product, by the oracle's plain ate pairing"""
    a, b, c = sh.rand_proof
    return o.pairing_product_is_one([
        (a, b),
        (G1.neg_affine(vk["alpha_g1"]), vk["beta_g2"]),
        (G1.neg_affine(prepared_inputs(vk, io_types, sh)), vk["gamma_g2"]),
        (G1.neg_affine(c), vk["delta_g2"]),
    ])


def accepts(pvk, vk, io_types, sh: Show) -> bool:
    """the same verdict through the oracle's restatement of ark's optimal-ate path (oracle/ark_files.py): much faster"""
    return ark_files.verify_proof_with_prepared_inputs(pvk, sh.rand_proof, prepared_inputs(vk, io_types, sh))


def k_bytes(ks) -> bytes:
    return b"".join(o.g1_compressed(P) for P in ks)


def ark_bytes(sh: Show) -> bytes:
    """ShowGroth16::serialize_uncompressed (groth16rand.rs:38-45; DLogPoK dlog.rs:16-20), written independently of the
    package: rand_proof | com_hidden_inputs | c | s: Vec<Vec<Fr>> | commited_inputs: Vec<G1>"""
    out = o.proof_uncompressed(sh.rand_proof) + o.g1_uncompressed(sh.com_hidden) + o.fe_bytes(sh.c)
    out += struct.pack("<Q", len(sh.s))
    for si in sh.s:
        out += struct.pack("<Q", len(si)) + b"".join(o.fe_bytes(x) for x in si)
    out += struct.pack("<Q", len(sh.committed)) + b"".join(o.g1_uncompressed(P) for P in sh.committed)
    return out


def api_show(cc, sh: Show):
    """(cc.ShowGroth16, revealed inputs) as Groth16.verify_show_batch takes them"""
    return (cc.ShowGroth16(o.proof_uncompressed(sh.rand_proof), o.g1_uncompressed(sh.com_hidden), sh.c, [list(si) for si in sh.s],
                           [o.g1_uncompressed(P) for P in sh.committed]), list(sh.revealed))


def jwt_like_layout(ell):
    """two committed inputs, several hidden ones, the rest revealed - the shape of Crescent's JWT proof spec"""
    io = [REVEALED] * ell
    for i in range(min(ell, 2)):
        io[i] = COMMITTED
    for i in range(2, min(ell, 2 + max(1, ell // 4))):
        io[i] = HIDDEN
    return io


# ---- value-level vectors for showings (tests/test_verify_values_cpu.py, tests/test_gpu_verify_values.py) ---------------
def clone(sh: Show, **kw) -> Show:
    d = dict(rand_proof=sh.rand_proof, com_hidden=sh.com_hidden, committed=list(sh.committed), c=sh.c, s=[list(si) for si in sh.s],
             revealed=list(sh.revealed))
    d.update(kw)
    return Show(**d)


# challenges around the ends of k_show_terms' double-and-add: it starts at bit 253, make_show draws c < 2^248
C_VALUES = [0, 1, (1 << 248) - 1, 1 << 253, R - 1]


def pattern_showings(sh: Show, patterns):
    """len(patterns) copies of an accepting showing with c overwritten by C_VALUES in rotation and response j of copy v by
    pattern (j + v) mod len(patterns): every response table meets every pattern.  No valid proofs of knowledge, and they
    need not be: the Groth16 verdict depends on neither c nor s, and k is whatever dlog.rs:137-145 recomputes."""
    out = []
    for v in range(len(patterns)):
        s, j = [], 0
        for si in sh.s:
            s.append([patterns[(j + t + v) % len(patterns)][1] for t in range(len(si))])
            j += len(si)
        out.append(clone(sh, c=C_VALUES[v % len(C_VALUES)], s=s))
    return out


def check_chain(vk, io_types, sh: Show):
    """k_show_check's chain: gamma_abc[0] + com_hidden + committed points + revealed partials -> (events, prepared inputs)"""
    import verify_vectors as V
    gabc = vk["gamma_abc_g1"]
    rev = [gabc[i + 1] for i, t in enumerate(io_types) if t == REVEALED]
    return V.chain_events(gabc[0], [sh.com_hidden] + list(sh.committed) + [_aff(_mul(P, x)) for P, x in zip(rev, sh.revealed)])


def k_chain(vk, io_types, sh: Show, i):
    """k_show_k's chain of statement i: c·y_i + s_i0·base_i0 + s_i1·base_i1 + ... -> (events, k_i)"""
    import verify_vectors as V
    bases = verifier_bases(vk, io_types)[i]
    return V.chain_events(_aff(_mul(sh.y[i], sh.c)), [_aff(_mul(P, s)) for P, s in zip(bases, sh.s[i])])


def coincident_show_cases():
    """honest (accepting) showings under one gamma = 1 key and the layout [C, C, H, R, R, R] whose partial sums coincide
    inside k_show_check's chain or inside one statement's k_show_k chain, by the choice of z, the commitment randomness or
    the nonces.  Returns (vk, io_types, two ordinary showings, [(name, Show, chain, expected events, final sum is O)]) with
    chain = "check" or the statement index."""
    import random
    import verify_vectors as V
    rng = random.Random(0x5C01)
    inv = lambda v: pow(v, R - 2, R)
    alpha, beta, delta = (rng.randrange(1, R) for _ in range(3))
    ks = [rng.randrange(1, R) for _ in range(7)]
    xs = [rng.randrange(1, R) for _ in range(6)]
    sc = (alpha, beta, 1, delta, ks)
    vk = V.synthetic_vk(*sc[:4], ks)
    proof = V.synthetic_proof(sc, xs, a=rng.randrange(1, R), b=rng.randrange(1, R))
    io = jwt_like_layout(6)
    assert io == [COMMITTED, COMMITTED, HIDDEN, REVEALED, REVEALED, REVEALED]
    di = inv(delta)
    r0, r1, z, c = rng.randrange(1, R), rng.randrange(1, R), rng.randrange(1, R), rng.randrange(1, 1 << 248)
    hid = lambda zz: (xs[2] * ks[3] + zz * delta) % R          # com_hidden's scalar
    y0 = lambda rr: (xs[0] * ks[1] + rr * delta) % R           # committed[0]'s scalar
    y1 = (xs[1] * ks[2] + r1 * delta) % R
    show = lambda **kw: make_show(vk, proof, xs, io, rng, **dict(dict(rs=[r0, r1], z=z, c=c), **kw))
    ordinary = [make_show(vk, proof, xs, io, rng), make_show(vk, proof, xs, io, rng)]
    cases = []
    # k_show_check: g0, then madd(com_hidden), madd(committed[0]), madd(committed[1]), add(revealed partials)
    cases.append(("com_hidden = g0: madd's dbl_affine branch", show(z=(ks[0] - xs[2] * ks[3]) * di % R), "check",
                  ["double", "add", "add", "add", "add", "add"], False))
    cases.append(("com_hidden = -g0: O, then committed[0] restarts the chain", show(z=(-ks[0] - xs[2] * ks[3]) * di % R), "check",
                  ["cancel", "restart", "add", "add", "add", "add"], False))
    cases.append(("committed[0] = g0 + com_hidden", show(rs=[(ks[0] + hid(z) - xs[0] * ks[1]) * di % R, r1]), "check",
                  ["add", "double", "add", "add", "add", "add"], False))
    zz = (xs[3] * ks[4] - ks[0] - xs[2] * ks[3] - y0(r0) - y1) * di % R
    cases.append(("the first revealed partial equals the running sum", show(z=zz), "check",
                  ["add", "add", "add", "double", "add", "add"], False))
    # k_show_k: c·y, then add(s_0·base_0), add(s_1·base_1), with s_j = rho_j - c·secret_j
    for stmt, base0, secret0, secret1, ysc, what in ((0, ks[1], xs[0], r0, y0(r0), "committed statement 0"),
                                                      (2, ks[3], xs[2], z, hid(z), "the hidden statement")):
        cy = c * ysc % R
        rho1 = rng.randrange(1, R)
        s1 = (rho1 - c * secret1) % R
        assert s1
        s0 = cy * inv(base0) % R
        cases.append(("%s: s_0 base_0 = c y, a doubling at the first add" % what, show(rho={stmt: [(s0 + c * secret0) % R, rho1]}),
                      stmt, ["double", "add"], False))
        cases.append(("%s: s_0 base_0 = -c y, s_1 base_1 != O: O mid-chain, k != O" % what,
                      show(rho={stmt: [(-s0 + c * secret0) % R, rho1]}), stmt, ["cancel", "restart"], False))
    rho0 = rng.randrange(1, R)
    s0 = (rho0 - c * xs[2]) % R
    cy = c * hid(z) % R
    s1 = (cy + s0 * ks[3]) * di % R
    cases.append(("the hidden statement: s_1 base_1 = c y + s_0 base_0, a doubling at the second add",
                  show(rho={2: [rho0, (s1 + c * z) % R]}), 2, ["add", "double"], False))
    s1 = (cy - s0 * ks[3]) * di % R
    cases.append(("the hidden statement: s_0 base_0 + s_1 base_1 = c y, so k = 2 c y by plain additions",
                  show(rho={2: [rho0, (s1 + c * z) % R]}), 2, ["add", "add"], False))
    return vk, io, ordinary, cases


def pattern_show_base():
    """(vk, io_types, an accepting showing) for pattern_showings: the `mixed` layout with ell = 6 under a gamma = 1 key"""
    import verify_vectors as V
    rng, sc = V.synthetic_scalars(6, 0x5A77, gamma=1)
    xs = [rng.randrange(R) for _ in range(6)]
    vk = V.synthetic_vk(*sc[:4], sc[4])
    proof = V.synthetic_proof(sc, xs, a=rng.randrange(1, R), b=rng.randrange(1, R))
    io = jwt_like_layout(6)
    return vk, io, make_show(vk, proof, xs, io, rng)
