"""Test vectors for creating showings (csrc/verify.hip, cg_show_commit_batch / cg_show_respond_batch): a
`show_vectors.Show` made with every random value explicit, next to the flat arrays the two entries take and the bytes they
must return.  Built with the oracle only.  Shared by tests/test_show_create_cpu.py and tests/test_gpu_show_create.py."""
import functools
from dataclasses import dataclass

import numpy as np

import bn254_oracle as o
import show_vectors as S
import verify_vectors as V

R, Q = o.R, o.Q
MADE, MALFORMED = 1, 2
LAYOUTS = ["revealed", "hidden", "committed", "mixed"]


def layout(name, ell):
    return {"revealed": [S.REVEALED] * ell, "hidden": [S.HIDDEN] * ell, "committed": [S.COMMITTED] * ell,
            "mixed": S.jwt_like_layout(ell)}[name]


def counts(io):
    """(n_committed, n_hidden, n_resp, n_rand)"""
    n_com, n_hid = io.count(S.COMMITTED), io.count(S.HIDDEN)
    n_resp = 2 * n_com + n_hid + 1
    return n_com, n_hid, n_resp, 3 + n_com + n_resp


def fe(xs) -> bytes:
    return b"".join(int(x).to_bytes(32, "little") for x in xs)


@dataclass
class Made:
    """one client state, the randomness of one showing of it, and what show_groth16 makes of them"""
    proof: tuple
    inputs: list
    rand: list            # r1, r2, the r_i, z, the nonces statement-major: one row of cg_show_commit_batch's `rand`
    show: object          # show_vectors.Show, None for a row that is expected to be malformed
    proof_bytes: bytes = None

    def __post_init__(self):
        if self.proof_bytes is None:
            self.proof_bytes = o.proof_uncompressed(self.proof)


def draw(io, rng, r1=None, r2=None, rs=None, z=None, rho=None):
    """the random values of one showing, explicit ones kept; rho: {statement: nonces}"""
    n_com, n_hid, _, _ = counts(io)
    r1 = rng.randrange(1, R) if r1 is None else r1
    r2 = rng.randrange(1, R) if r2 is None else r2
    rs = [rng.randrange(R) for _ in range(n_com)] if rs is None else list(rs)
    z = rng.randrange(R) if z is None else z
    shapes = [2] * n_com + [n_hid + 1]
    rho = dict(rho or {})
    for i, k in enumerate(shapes):
        if i not in rho:
            rho[i] = [rng.randrange(R) for _ in range(k)]
        assert len(rho[i]) == k
    return dict(r1=r1, r2=r2, rs=rs, z=z, rho=rho)


def rand_row(io, d):
    n_com = counts(io)[0]
    return [d["r1"], d["r2"]] + list(d["rs"]) + [d["z"]] + [x for i in range(n_com + 1) for x in d["rho"][i]]


def make(vk, proof, xs, io, rng, c=None, **kw) -> Made:
    d = draw(io, rng, **kw)
    sh = S.make_show(vk, proof, xs, io, rng, c=c, **d)
    row = rand_row(io, d)
    assert len(row) == counts(io)[3]
    return Made(proof, list(xs), row, sh)


def pack(made):
    """(proofs, inputs, rand) of cg_show_commit_batch, one row per client state"""
    rows = lambda parts: np.stack([np.frombuffer(p, np.uint8) for p in parts])
    return rows([m.proof_bytes for m in made]), rows([fe(m.inputs) for m in made]), rows([fe(m.rand) for m in made])


def expected(io, m: Made):
    """(rand_proof 256 B, com_hidden 64 B, committed, k, s) as the two entries must write them; zeros for a malformed row"""
    n_com, _, n_resp, _ = counts(io)
    if m.show is None:
        return bytes(256), bytes(64), bytes(64 * n_com), bytes(32 * (n_com + 1)), bytes(32 * n_resp)
    sh = m.show
    return (o.proof_uncompressed(sh.rand_proof), o.g1_uncompressed(sh.com_hidden), b"".join(o.g1_uncompressed(P) for P in sh.committed),
            S.k_bytes(sh.k), fe([x for si in sh.s for x in si]))


def synthetic(ell, seed, gamma=1):
    """a key from chosen non-zero scalars, inputs and an accepting proof with its scalars (a, b, c)"""
    rng, sc = V.synthetic_scalars(ell, seed, gamma=gamma)
    xs = [rng.randrange(R) for _ in range(ell)]
    abc = V.solve_proof_scalars(sc, V.prepared_scalar(sc[4], xs), a=rng.randrange(1, R), b=rng.randrange(1, R))
    return rng, sc, V.synthetic_vk(*sc[:4], sc[4]), xs, abc


def proof_of(abc):
    return (V.g1(abc[0]), V.g2(abc[1]), V.g1(abc[2])) if all(abc) else \
        tuple(None if s == 0 else f(s) for f, s in zip((V.g1, V.g2, V.g1), abc))


ALL_FF = V._alternating(0xFF, 0xFF)          # every 8-bit window 0xFF, the top one capped at 0x2F: below r


@functools.lru_cache(maxsize=None)
def edge_cases():
    """(vk, io, [(name, Made, the outputs that must be O)]) on one key with known scalars and the layout [C, C, H, R, R, R]:
    randomness chosen so that a partial sum of cg_show_commit_batch's chains is O, or two of its operands coincide.
    Outputs are named "A", "B", "C", "com_hidden", "committed0", "k0"."""
    rng, sc, vk, xs, (a, b, c) = synthetic(6, 0xED6E)
    io = S.jwt_like_layout(6)
    assert io == [S.COMMITTED, S.COMMITTED, S.HIDDEN, S.REVEALED, S.REVEALED, S.REVEALED]
    delta, ks = sc[3], sc[4]
    inv = lambda v: pow(v % R, R - 2, R)
    di = inv(delta)
    proof = proof_of((a, b, c))
    r2, r0, r1c, z = (rng.randrange(1, R) for _ in range(4))       # the defaults the cases below vary
    cases = []

    def case(name, zero=(), proof=proof, **kw):
        kw = dict(dict(r2=r2, rs=[r0, r1c], z=z), **kw)
        m = make(vk, proof, xs, io, rng, **kw)
        cases.append((name, m, tuple(zero)))

    case("r1 = 1", r1=1)
    case("r1 = r - 1", r1=R - 1)
    case("r2 = -b/delta: B + r2 delta_g2 = O", zero=["B"], r2=-b * di % R)
    case("r2 = -c/a: C + r2 A = O before the generator term", r2=-c * inv(a) % R)
    case("r2 = c/a: r2 A = C, a doubling", r2=c * inv(a) % R)
    case("z = c + r2 a - sum r_i: C'' = O", zero=["C"], z=(c + r2 * a - r0 - r1c) % R)
    case("sum r_i + z = 0: the generator term is O", z=-(r0 + r1c) % R)
    case("r_0 = x_0 k_1/delta: the two terms of committed[0] are equal", rs=[xs[0] * ks[1] * di % R, r1c])
    case("r_0 = -x_0 k_1/delta: committed[0] = O", zero=["committed0"], rs=[-xs[0] * ks[1] * di % R, r1c])
    case("z = -x_2 k_3/delta: com_hidden = O", zero=["com_hidden"], z=-xs[2] * ks[3] * di % R)
    K = V.prepared_scalar(ks, xs)
    for name, zero, abc in (("proof A = O", ["A"], V.solve_proof_scalars(sc, K, a=0, b=b)),
                            ("proof B = O: B' = r1 r2 delta_g2", [], V.solve_proof_scalars(sc, K, a=a, b=0)),
                            ("proof C = O", [], V.solve_proof_scalars(sc, K, a=a, c=0))):
        case(name, zero=zero, proof=proof_of(abc))
    t = rng.randrange(1, R)
    case("nonces (t, -t k_1/delta) of statement 0: k_0 = O", zero=["k0"], rho={0: [t, -t * ks[1] * di % R]})
    case("every window 0xFF as r_0 and as a nonce", rs=[ALL_FF, r1c], rho={1: [ALL_FF, rng.randrange(R)], 2: [rng.randrange(R), ALL_FF]})
    return vk, io, cases


def outputs_that_are_o(m: Made):
    sh = m.show
    out = [n for n, P in zip("ABC", sh.rand_proof) if P is None]
    if sh.com_hidden is None:
        out.append("com_hidden")
    out += ["committed%d" % i for i, P in enumerate(sh.committed) if P is None]
    out += ["k%d" % i for i, P in enumerate(sh.k) if P is None]
    return tuple(out)
