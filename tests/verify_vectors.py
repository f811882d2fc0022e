"""Test vectors for Groth16 verification (csrc/pairing.hpp, csrc/verify.hip), built with the oracle only: Fq12 / G2
helpers, twist points outside G2, synthetic keys from chosen scalars, and the golden circuits' verifying keys.  Shared by
tests/test_pairing_host.py, tests/test_verify_cpu.py and tests/test_gpu_verify.py."""
import random

import ark_files
import bn254_oracle as o
from conftest import load_golden

Q, R = o.Q, o.R
F2 = o.Fq2Ops


def fq2_pow(a, e):
    r = F2.one
    for bit in bin(e)[2:]:
        r = F2.sqr(r)
        if bit == "1":
            r = F2.mul(r, a)
    return r


def fq2_sqrt(a):
    """square root in Fq2 for q = 3 (mod 4) (Adj, Rodriguez-Henriquez, alg. 9); None when a is not a square"""
    a1 = fq2_pow(a, (Q - 3) // 4)
    alpha = F2.mul(a1, F2.mul(a1, a))
    a0 = F2.mul((alpha[0], (-alpha[1]) % Q), alpha)
    if a0 == (Q - 1, 0):
        return None
    x0 = F2.mul(a1, a)
    if alpha == (Q - 1, 0):
        x = F2.mul((0, 1), x0)
    else:
        x = F2.mul(fq2_pow(F2.add(F2.one, alpha), (Q - 1) // 2), x0)
    return x if F2.sqr(x) == a else None


def twist_point_outside_g2(rng):
    """a point on the twist y^2 = x^3 + b' whose order is not r"""
    while True:
        x = (rng.randrange(Q), rng.randrange(Q))
        y = fq2_sqrt(F2.add(F2.mul(F2.sqr(x), x), o.B2))
        if y is None:
            continue
        P = (x, y)
        if o.G2.to_affine(o.G2.mul_affine(P, R)) is not None:
            return P


def random_f12(rng):
    return [rng.randrange(Q) for _ in range(12)]


def g1(k):
    return o.G1.to_affine(o.G1.mul_affine(o.G1_GEN, k % R))


def g2(k):
    return o.G2.to_affine(o.G2.mul_affine(o.G2_GEN, k % R))


def g1_hex(P):
    return o.g1_packed(P).hex()


def g2_hex(P):
    return o.g2_packed(P).hex()


def vk_bytes(vk) -> bytes:
    return o.vk_uncompressed(vk)


def synthetic_vk(alpha, beta, gamma, delta, ks):
    """a VerifyingKey from chosen scalars: gamma_abc_g1[i] = k_i·G1"""
    return dict(alpha_g1=g1(alpha), beta_g2=g2(beta), gamma_g2=g2(gamma), delta_g1=g1(delta), delta_g2=g2(delta),
                gamma_abc_g1=[g1(k) for k in ks])


def solve_proof_scalars(sc, K, a=None, b=None, c=None):
    """(a, b, c) with ab = alpha beta + K gamma + c delta for a prepared-input scalar K given directly; exactly one of a, b,
    c may be left None and is solved for"""
    alpha, beta, gamma, delta = sc[:4]
    rhs0 = (alpha * beta + K * gamma) % R
    if c is None:
        c = (a * b - rhs0) * pow(delta, R - 2, R) % R
    elif b is None:
        b = (rhs0 + c * delta) * pow(a, R - 2, R) % R
    elif a is None:
        a = (rhs0 + c * delta) * pow(b, R - 2, R) % R
    assert equation_holds(sc, K, a, b, c)
    return a % R, b % R, c % R


def equation_holds(sc, K, a, b, c) -> bool:
    """the Groth16 check in the exponent: e(A, B) = e(alpha, beta) e(K G1, gamma) e(C, delta)"""
    alpha, beta, gamma, delta = sc[:4]
    return (a * b - alpha * beta - K * gamma - c * delta) % R == 0


def prepared_scalar(ks, inputs):
    return (ks[0] + sum(x * k for x, k in zip(inputs, ks[1:]))) % R


def synthetic_proof_for_k(sc, K, a=None, b=None, c=None):
    """(A, B, C) = (a G1, b G2, c G1) for the prepared-input scalar K: what a showing needs, whose prepared inputs are
    g0 + com_hidden + sum committed + sum revealed rather than k_0 + sum x_i k_i"""
    a, b, c = solve_proof_scalars(sc, K, a, b, c)
    return (g1(a), g2(b), g1(c))


def synthetic_proof(sc, inputs, a=None, b=None, c=None):
    """(A, B, C) = (a G1, b G2, c G1) with ab = alpha beta + (k_0 + sum x_i k_i) gamma + c delta; exactly one of a, b, c
    may be left None and is solved for (a = 0, b = 0 or c = 0 give the identity)"""
    return synthetic_proof_for_k(sc, prepared_scalar(sc[4], inputs), a, b, c)


def proof_bytes(pr) -> bytes:
    return o.proof_uncompressed(pr)


def inputs_bytes(xs) -> bytes:
    return b"".join(int(x).to_bytes(32, "little") for x in xs)


def golden_vk(name):
    """(vk, public inputs, [(r, s, proof bytes)]) of a golden circuit; the key is regenerated from its trapdoor"""
    g = load_golden("groth16_%s.json" % name)
    t = g["trapdoor"]
    if "dummy" in g:
        d = g["dummy"]
        mats, l, m, M, w = o.dummy_circuit(int(d["a"], 16), int(d["b"], 16), d["num_variables"], d["num_constraints"], d["num_inputs"])
    else:
        mats = tuple([[(int(c, 16), col) for c, col in row] for row in mat] for mat in g["matrices"])
        l, m, M = g["num_inputs"], g["num_constraints"], g["num_variables"]
        w = [int(x, 16) for x in g["witness"]]
    pk, _ = o.generate_parameters(mats, l, m, M, int(t["tau"], 16), int(t["alpha"], 16), int(t["beta"], 16), int(t["delta"], 16))
    return pk, mats, w, g


def oracle_pvk_bytes(vk) -> bytes:
    return ark_files.pvk_bytes(ark_files.prepare_verifying_key(vk))


def rng(seed):
    return random.Random(seed)


# ---- value-level vectors for the verifier (tests/test_verify_values_cpu.py, tests/test_gpu_verify_values.py) -----------
def _alternating(even, odd):
    """32 little-endian bytes, `even` in windows 0, 2, ... and `odd` in windows 1, 3, ...; a top window of 0xFF would
    pass r (its top byte is 0x30), so it holds 0x2F, the largest digit under which any lower bytes stay below r"""
    b = bytearray([even, odd] * 16)
    if b[31] == 0xFF:
        b[31] = 0x2F
    return int.from_bytes(bytes(b), "little")


# scalars below r that steer the 8-bit fixed-base digit walk: zero bytes inside a scalar, digit 255, the top window and its
# largest legal digit 0x30, one-window scalars, r - 1.  The random one is drawn at full width (bit 253 set).
DIGIT_PATTERNS = [
    ("0", 0),
    ("1", 1),
    ("255", 255),
    ("256", 256),
    ("2^248", 1 << 248),
    ("0x30*2^248", 0x30 << 248),
    ("2^253", 1 << 253),
    ("r-1", R - 1),
    ("0x2F then 31 bytes 0xFF", (0x2F << 248) | ((1 << 248) - 1)),
    ("alternating 00 FF", _alternating(0x00, 0xFF)),
    ("alternating FF 00", _alternating(0xFF, 0x00)),
    ("random full width", random.Random(0xD161).randrange(1 << 253, R)),
]
assert all(0 <= v < R for _, v in DIGIT_PATTERNS)


def _multiples(scalars, cc, group):
    """scalar·generator for non-zero scalars, affine: from the package's fixed-base kernels when cc is given (pinned to the
    oracle by tests/test_gpu_parity.py::test_fixed_base_vs_oracle), by the oracle's own multiplication otherwise"""
    if cc is None:
        return [(g1 if group == 1 else g2)(k) for k in scalars]
    width = 64 * group
    out = (cc.fixed_base_g1 if group == 1 else cc.fixed_base_g2)(inputs_bytes(scalars))
    unpack = o.g1_unpack if group == 1 else o.g2_unpack
    return [unpack(out[width * i:width * (i + 1)]) for i in range(len(scalars))]


def distinct_proofs(sc, n, rng, cc=None):
    """n distinct accepting proofs under one synthetic key: per proof its own a_i, b_i and inputs, c_i solved for, all of
    a_i, b_i, c_i non-zero.  Returns (inputs, [(a, b, c)] scalars, [(A, B, C)] affine)."""
    ell = len(sc[4]) - 1
    inputs, scalars = [], []
    while len(scalars) < n:
        xs = [rng.randrange(R) for _ in range(ell)]
        a, b, c = solve_proof_scalars(sc, prepared_scalar(sc[4], xs), a=rng.randrange(1, R), b=rng.randrange(1, R))
        if c:
            inputs.append(xs)
            scalars.append((a, b, c))
    A = _multiples([s[0] for s in scalars], cc, 1)
    B = _multiples([s[1] for s in scalars], cc, 2)
    C = _multiples([s[2] for s in scalars], cc, 1)
    assert len({p for p in A}) == len({p for p in B}) == len({p for p in C}) == n and None not in A + B + C
    return inputs, scalars, list(zip(A, B, C))


TAMPERINGS = ["input (i mod 3) plus 1", "A of slot i+1", "B of slot i+1", "C of slot i+1"]


def interleave_tampered(sc, inputs, scalars, proofs):
    """the same batch with every odd slot i tampered in one of the four TAMPERINGS, in rotation, and every even slot
    untouched.  The verdict of every slot follows from ab = alpha beta + K gamma + c delta mod r, asserted here: it holds on
    the even slots and fails on the odd ones.  Returns (inputs, proofs, tampering per slot or None)."""
    n = len(proofs)
    out_in, out_pr, how = [], [], []
    for i in range(n):
        xs, (a, b, c), (A, B, C) = list(inputs[i]), scalars[i], proofs[i]
        nxt = (i + 1) % n
        kind = None
        if i & 1:
            kind = (i // 2) % 4
            if kind == 0:
                xs[i % 3] = (xs[i % 3] + 1) % R
            elif kind == 1:
                a, A = scalars[nxt][0], proofs[nxt][0]
            elif kind == 2:
                b, B = scalars[nxt][1], proofs[nxt][1]
            else:
                c, C = scalars[nxt][2], proofs[nxt][2]
        assert equation_holds(sc, prepared_scalar(sc[4], xs), a, b, c) == (kind is None), i
        out_in.append(xs)
        out_pr.append((A, B, C))
        how.append(None if kind is None else TAMPERINGS[kind])
    return out_in, out_pr, how


def digit_pattern_proofs(sc, rng, cc=None):
    """for a key with ell = len(DIGIT_PATTERNS): proof p takes pattern (j + p) mod ell as its input j, so every table meets
    every pattern.  Returns (inputs, accepting proofs, bumped inputs): the bumped row of proof p has the input at position
    -2p mod ell plus 1 mod r, which the same proof no longer satisfies.  That input holds pattern -p mod ell, so every
    pattern is bumped once (r - 1 becomes 0)."""
    ell = len(sc[4]) - 1
    assert ell == len(DIGIT_PATTERNS) and all(sc[4])
    inputs = [[DIGIT_PATTERNS[(j + p) % ell][1] for j in range(ell)] for p in range(ell)]
    scalars = [solve_proof_scalars(sc, prepared_scalar(sc[4], xs), a=rng.randrange(1, R), b=rng.randrange(1, R)) for xs in inputs]
    assert all(c for _, _, c in scalars)
    proofs = list(zip(_multiples([s[0] for s in scalars], cc, 1), _multiples([s[1] for s in scalars], cc, 2),
                      _multiples([s[2] for s in scalars], cc, 1)))
    bumped = []
    for p, (xs, (a, b, c)) in enumerate(zip(inputs, scalars)):
        ys = list(xs)
        ys[-2 * p % ell] = (ys[-2 * p % ell] + 1) % R
        assert not equation_holds(sc, prepared_scalar(sc[4], ys), a, b, c)
        bumped.append(ys)
    return inputs, proofs, bumped


def chain_events(start, operands):
    """acc = start; acc += P for every operand, walked with the oracle on affine points as the kernels walk it in XYZZ.
    Per step: 'skip' (P = O), 'restart' (acc = O, acc becomes P), 'double' (acc = P), 'cancel' (acc = -P, acc becomes O)
    or 'add'.  Returns (events, the final sum affine)."""
    acc, events = start, []
    for P in operands:
        if P is None:
            events.append("skip")
            continue
        if acc is None:
            events.append("restart")
        elif acc == P:
            events.append("double")
        elif acc == o.G1.neg_affine(P):
            events.append("cancel")
        else:
            events.append("add")
        acc = o.G1.to_affine(o.G1.add_affine(o.G1.to_jac(acc), P))
    return events, acc


def input_chain(vk, xs):
    """k_vfy_check's chain: gamma_abc[0] + x_1 gamma_abc[1] + ... -> (events, prepared inputs)"""
    gabc = vk["gamma_abc_g1"]
    return chain_events(gabc[0], [None if P is None else o.G1.to_affine(o.G1.mul_affine(P, x % R)) for P, x in zip(gabc[1:], xs)])


def coincident_input_cases():
    """proofs whose per-input partial sums coincide inside k_vfy_check's chain.  Each case: (name, key scalars, inputs, the
    expected events of the chain, whether the prepared inputs are O, an accepting proof, the same proof with another C)."""
    rng = random.Random(0xC01C)
    inv = lambda v: pow(v, R - 2, R)
    alpha, beta, gamma, delta = (rng.randrange(1, R) for _ in range(4))
    k0, k1, k2, k3 = ks = [rng.randrange(1, R) for _ in range(4)]
    sc = (alpha, beta, gamma, delta, ks)
    x1, x2, x3 = (rng.randrange(1, R) for _ in range(3))
    s1 = k0 + x1 * k1                                   # the running sum after a random first input
    cases = [
        ("x1 k1 = k0: the first add doubles the affine-lifted g0", sc, [k0 * inv(k1) % R, x2, x3], ["double", "add", "add"], False),
        ("x1 k1 = -k0: O mid-chain, x2 G2 restarts", sc, [-k0 * inv(k1) % R, x2, x3], ["cancel", "restart", "add"], False),
        ("x2 k2 = k0 + x1 k1: a doubling with zz != 1 on both sides", sc, [x1, s1 * inv(k2) % R, x3], ["add", "double", "add"], False),
        ("x2 k2 = -(k0 + x1 k1), then x3 != 0", sc, [x1, -s1 * inv(k2) % R, x3], ["add", "cancel", "restart"], False),
        ("x3 k3 cancels everything: prepared inputs O in the last step", sc, [x1, x2, -(s1 + x2 * k2) * inv(k3) % R],
         ["add", "add", "cancel"], True),
    ]
    # a second key: gamma_abc[0] = O, gamma_abc[1] = O under a non-zero input, gamma_abc[2] = gamma_abc[3] under equal inputs
    k = rng.randrange(1, R)
    sc2 = (alpha, beta, gamma, delta, [0, 0, k, k])
    cases.append(("g0 = O, gamma_abc[1] = O, gamma_abc[2] = gamma_abc[3] under equal inputs: a partial equals a partial", sc2,
                  [x1, x2, x2], ["skip", "restart", "double"], False))
    out = []
    for name, key, xs, events, pi_is_o in cases:
        K = prepared_scalar(key[4], xs)
        assert (K == 0) == pi_is_o
        a, b, c = solve_proof_scalars(key, K, a=rng.randrange(1, R), b=rng.randrange(1, R))
        assert c and not equation_holds(key, K, a, b, c + 1)
        out.append((name, key, xs, events, pi_is_o, (g1(a), g2(b), g1(c)), (g1(a), g2(b), g1(c + 1))))
    return out


def synthetic_scalars(ell, seed, gamma=None):
    """(rng, key scalars) with non-zero alpha, beta, gamma, delta and k_0 .. k_ell"""
    r = random.Random(seed)
    alpha, beta, g, delta = (r.randrange(1, R) for _ in range(4))
    return r, (alpha, beta, g if gamma is None else gamma, delta, [r.randrange(1, R) for _ in range(ell + 1)])
