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
