"""The crafted vectors of tests/test_gpu_verify_values.py are what they claim, without a GPU: every chain the verifier's
kernels walk (k_vfy_check, k_show_check, k_show_k in csrc/verify.hip) is walked with the oracle on affine points, the named
coincidence - a doubling, a cancellation to O, a restart from O - happens at the named step and the final sum is or is not
O as stated, and every crafted proof and showing gets the verdict the oracle's verifier gives it.  Vectors:
tests/verify_vectors.py, tests/show_vectors.py."""
import pytest

import ark_files
import bn254_oracle as o
import show_vectors as S
import verify_vectors as V

R = o.R


def _vk(sc):
    return V.synthetic_vk(*sc[:4], sc[4])


def test_digit_patterns_are_the_named_scalars():
    pat = dict(V.DIGIT_PATTERNS)
    assert len(V.DIGIT_PATTERNS) == len(pat) == 12 and all(0 <= v < R for v in pat.values())
    le = lambda name: pat[name].to_bytes(32, "little")
    assert [pat[k] for k in ("0", "1", "255", "256")] == [0, 1, 255, 256]
    assert le("2^248") == bytes(31) + b"\x01" and le("0x30*2^248") == bytes(31) + b"\x30" and le("2^253") == bytes(31) + b"\x20"
    assert pat["r-1"] + 1 == R and le("r-1")[31] == 0x30           # 0x30 is the top window's largest legal digit
    assert (0x31 << 248) > R > (0x30 << 248)
    assert le("0x2F then 31 bytes 0xFF") == b"\xff" * 31 + b"\x2f"
    assert le("alternating 00 FF") == b"\x00\xff" * 15 + b"\x00\x2f" and le("alternating FF 00") == b"\xff\x00" * 16
    assert pat["random full width"] >> 253 == 1


def test_a_proof_is_solved_for_a_prepared_input_scalar_given_directly():
    """synthetic_proof is synthetic_proof_for_k at K = k_0 + sum x_i k_i, and a K assembled as a showing assembles it
    (g0 + com_hidden + committed + revealed) gives a proof that showing's verifier accepts - here under gamma != 1"""
    rng, sc = V.synthetic_scalars(3, 21)
    xs = [rng.randrange(R) for _ in range(3)]
    a, b = rng.randrange(1, R), rng.randrange(1, R)
    assert V.synthetic_proof(sc, xs, a=a, b=b) == V.synthetic_proof_for_k(sc, V.prepared_scalar(sc[4], xs), a=a, b=b)
    ks = sc[4]
    io = [S.COMMITTED, S.HIDDEN, S.REVEALED]
    h, y = rng.randrange(1, R), rng.randrange(1, R)                   # any com_hidden and committed point
    K = (ks[0] + h + y + xs[2] * ks[3]) % R
    sh = S.Show(V.synthetic_proof_for_k(sc, K, a=a, b=b), V.g1(h), [V.g1(y)], 0, [[0, 0], [0, 0]], [xs[2]])
    vk = _vk(sc)
    assert S.prepared_inputs(vk, io, sh) == V.g1(K)
    assert S.accepts(ark_files.prepare_verifying_key(vk), vk, io, sh)


def test_distinct_proofs_and_their_tampered_slots():
    """the builder on a small n, by the oracle's own multiplication: distinct accepting proofs, and in the interleaved batch
    every tampering in turn, each with the verdict the builder derived mod r"""
    rng, sc = V.synthetic_scalars(3, 22)
    inputs, scalars, proofs = V.distinct_proofs(sc, 8, rng)
    assert len({V.proof_bytes(p) for p in proofs}) == 8 and len({tuple(x) for x in inputs}) == 8
    for (a, b, c), (A, B, C) in zip(scalars, proofs):
        assert a and b and c and (A, B, C) == (V.g1(a), V.g2(b), V.g1(c))
    t_in, t_pr, how = V.interleave_tampered(sc, inputs, scalars, proofs)
    assert how == [None, V.TAMPERINGS[0], None, V.TAMPERINGS[1], None, V.TAMPERINGS[2], None, V.TAMPERINGS[3]]
    assert t_in[1] != inputs[1] and t_pr[3][0] == proofs[4][0] and t_pr[5][1] == proofs[6][1] and t_pr[7][2] == proofs[0][2]
    pvk = ark_files.prepare_verifying_key(_vk(sc))
    assert ark_files.verify_with_processed_vk(pvk, inputs[1], proofs[1])
    for i in range(8):
        assert ark_files.verify_with_processed_vk(pvk, t_in[i], t_pr[i]) == (how[i] is None), i


def test_digit_pattern_proofs():
    rng, sc = V.synthetic_scalars(12, 23)
    inputs, proofs, bumped = V.digit_pattern_proofs(sc, rng)
    values = [v for _, v in V.DIGIT_PATTERNS]
    for j in range(12):                                                # every table meets every pattern
        assert sorted(xs[j] for xs in inputs) == sorted(values)
    changed = [[j for j in range(12) if xs[j] != ys[j]] for xs, ys in zip(inputs, bumped)]
    assert all(len(ch) == 1 for ch in changed)
    assert sorted(xs[ch[0]] for xs, ch in zip(inputs, changed)) == sorted(values)      # every pattern is bumped once
    assert any(xs[ch[0]] == R - 1 and ys[ch[0]] == 0 for xs, ys, ch in zip(inputs, bumped, changed))
    pvk = ark_files.prepare_verifying_key(_vk(sc))
    for p in range(12):
        assert ark_files.verify_with_processed_vk(pvk, inputs[p], proofs[p]), p
        assert not ark_files.verify_with_processed_vk(pvk, bumped[p], proofs[p]), p


@pytest.mark.parametrize("case", V.coincident_input_cases(), ids=lambda c: c[0].split(":")[0])
def test_coincident_input_chain(case):
    name, sc, xs, events, pi_is_o, good, bad = case
    vk = _vk(sc)
    got, pi = V.input_chain(vk, xs)
    assert got == events, name
    assert (pi is None) == pi_is_o and pi == o.G1.to_affine(o.prepare_inputs(vk, xs))
    pvk = ark_files.prepare_verifying_key(vk)
    assert ark_files.verify_with_processed_vk(pvk, xs, good)
    assert not ark_files.verify_with_processed_vk(pvk, xs, bad)


def test_coincident_show_chains():
    vk, io, ordinary, cases = S.coincident_show_cases()
    pvk = ark_files.prepare_verifying_key(vk)
    for sh in ordinary:
        assert S.accepts(pvk, vk, io, sh)
        assert "double" not in S.check_chain(vk, io, sh)[0] + sum((S.k_chain(vk, io, sh, i)[0] for i in range(3)), [])
    assert len({S.ark_bytes(sh) for _, sh, _, _, _ in cases}) == len(cases) == 10
    for name, sh, chain, events, final_is_o in cases:
        if chain == "check":
            got, end = S.check_chain(vk, io, sh)
            assert end == S.prepared_inputs(vk, io, sh), name
        else:
            got, end = S.k_chain(vk, io, sh, chain)
            assert end == S.recomputed_k(vk, io, sh)[chain] == sh.k[chain], name
        assert got == events, name
        assert (end is None) == final_is_o, name
        assert S.accepts(pvk, vk, io, sh), name


def test_pattern_showings():
    """c and the responses do not enter the Groth16 verdict: every copy keeps the base showing's proof and prepared inputs,
    so the oracle's one verdict on those (ACCEPT) is the verdict of each.  Their recomputed k have y of both signs."""
    vk, io, base = S.pattern_show_base()
    assert S.accepts(ark_files.prepare_verifying_key(vk), vk, io, base)
    shows = S.pattern_showings(base, V.DIGIT_PATTERNS)
    assert len(shows) == 12 and {sh.c for sh in shows} == set(S.C_VALUES) and base.c < 1 << 248
    values = sorted(v for _, v in V.DIGIT_PATTERNS)
    for j in range(6):
        assert sorted([x for si in sh.s for x in si][j] for sh in shows) == values
    pi = S.prepared_inputs(vk, io, base)
    flags = set()
    for sh in shows:
        assert sh.rand_proof == base.rand_proof and S.prepared_inputs(vk, io, sh) == pi
        flags |= {o.g1_compressed(P)[31] & 0xC0 for P in S.recomputed_k(vk, io, sh)}
    assert {0x00, 0x80} <= flags
