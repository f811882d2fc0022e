"""What tests/test_gpu_key_degenerate.py stands on, checked without a GPU (tests/degenerate_keys.py):

  * the walk of k_ec_stage's network over logarithms gives the inverse DFT of the definition;
  * the restated fold and h transform (msm.hpp, identities (1) and (2)) give the C part of the closed-form proof;
  * the closed-form proof is the oracle's proof on hand-made keys;
  * every family of keys reaches the events it is aimed at - the counts are asserted here, event by event, so that no GPU
    case claims a branch that its key does not take.  A generic key takes none of them."""
import random

import pytest

import degenerate_keys as dk

R = dk.R


@pytest.fixture(scope="module")
def circ64():
    return dk.Circuit(64)


# ------------------------------------------------------------------------------------------------- the shadows
@pytest.mark.parametrize("logn", [1, 2, 6])
def test_shadow_transform_is_the_direct_sum(logn):
    rng = random.Random(logn)
    n = 1 << logn
    total = (n >> 1) * logn
    for kind in ("random", "with identities", "family"):
        if kind == "random":
            x = [rng.randrange(1, R) for _ in range(n)]
        elif kind == "with identities":
            x = [rng.randrange(1, R) if rng.random() < 0.5 else 0 for _ in range(n)]
        else:
            x = dk.family_sequence("constant", logn)
        out, ev = dk.shadow_inverse_dft(x, logn)
        assert out == dk.direct_inverse_dft(x, logn), kind
        assert sum(ev[e] for e in dk.DFT_EVENTS) == total                  # one event per butterfly
        if kind == "random":
            assert ev["generic"] == total and ev["identity_outputs"] == 0


def test_a_generic_key_reaches_one_vinf_and_nothing_else(circ64):
    """what every key made from a random trapdoor gives the two transforms: the missing last point, met once"""
    h = dk.generic_h(6)
    for ev in (dk.shadow_h_transform(h, 6)[1], dk.shadow_fold(h, 6, circ64.mats[2], circ64.base_key().l, 2, circ64.M)["dft"]):
        assert ev["v_identity"] == 1 and ev["generic"] == 191
        assert not any(ev[e] for e in ("u_identity_v_finite", "u_eq_t_k0", "u_eq_t_k", "u_eq_neg_t_k0", "u_eq_neg_t_k",
                                       "identity_between_stages", "identity_outputs"))


def _coset_products(mats, l, m, w):
    """q_j = vinv·a(g ω^j)·b(g ω^j): the scalars of the h MSM over the transformed query (r1cs_to_qap.rs:164-187)"""
    o = dk.o
    D = o.domain_size_for(m + l)
    a = [o.evaluate_constraint(mats[0][i], w) for i in range(m)] + [w[i] for i in range(l)] + [0] * (D - m - l)
    b = [o.evaluate_constraint(mats[1][i], w) for i in range(m)] + [0] * (D - m)
    vinv = dk.inv(o.evaluate_vanishing_polynomial(D, o.FR_GENERATOR))
    return [vinv * x % R * y % R for x, y in zip(o.coset_fft(o.ifft(a)), o.coset_fft(o.ifft(b)))]


@pytest.mark.parametrize("D", [2, 4, 64])
def test_shadow_fold_and_h_transform_give_the_closed_form(D):
    """Σ_j q_j·H'_j + Σ_k w_k·folded_k = <w[l:], l> + <h, h_query>: the shadows restate what the library loads, and the closed
    form what it must prove, for an assignment that does not satisfy the system"""
    circ = dk.Circuit(D)
    key = circ.base_key().replace(h=dk.generic_h(circ.logn))
    Ht, _ = dk.shadow_h_transform(key.h, circ.logn)
    f = dk.shadow_fold(key.h, circ.logn, circ.mats[2], key.l, circ.l, circ.M)
    for w in circ.witnesses().values():
        q = _coset_products(circ.mats, circ.l, circ.m, w)
        hc = dk.o.witness_map_from_matrices(circ.mats, circ.l, circ.m, w)
        assert (dk.dot(q, Ht) + dk.dot(w, f["folded"])) % R == (dk.dot(w[circ.l:], key.l) + dk.dot(hc, key.h)) % R


# ------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("which", ["constant h query, D = 64", "identity and repeated l points, D = 4"])
def test_closed_form_is_the_oracles_proof(which):
    o = dk.o
    if which.startswith("constant"):
        circ = dk.Circuit(64)
        key = circ.base_key().replace(h=[12345] * 63)
    else:
        circ = dk.Circuit(4)
        key = circ.base_key()
        assert key.l[0] == 0 and key.l[1] == key.l[2]
        key = key.replace(h=dk.generic_h(2))
    pk = dk.oracle_key(key)
    assert all(o.G1.is_on_curve(p) for p in pk["h_query"] + pk["l_query"] + pk["a_query"])
    assert pk["l_query"][0] is None and (which.startswith("constant") or pk["l_query"][1] == pk["l_query"][2])
    rng = random.Random(5)
    for name, w in circ.witnesses().items():
        for r, s in ((0, 0), (rng.randrange(1, R), rng.randrange(1, R))):
            want = o.proof_uncompressed(o.create_proof_with_reduction_and_matrices(pk, r, s, circ.mats, circ.l, circ.m, w))
            assert dk.closed_form_proof(key, circ.mats, circ.m, w, r, s) == want, (name, r != 0)


# ------------------------------------------------------------------------------------------------- the families
# What each case of the GPU file claims, counted on the very key it loads (dk.case_key).  `aimed` is the transform the family was
# scaled for: its butterflies see the named sequence; the other transform sees the same points under other factors.
def _aimed(name):
    Ht, evh, f = dk.case_events(name)
    return (f["G"], f["dft"], f) if dk.CASES[name][2] == "fold" else (Ht, evh, f)


_TOTAL = 32 * 6


@pytest.mark.parametrize("name", ["constant/h", "constant/fold"])
def test_constant_family(name):
    """doubling (and, in the other output, cancellation) at k = 0, then identity operands on either side"""
    out, ev, f = _aimed(name)
    assert ev["u_eq_t_k0"] == 57 and ev["u_identity_v_finite"] == 57 and ev["v_identity"] == 73 and ev["identity_between_stages"] == 201


def test_single_point_families():
    Ht, evh, f = dk.case_events("index0")
    for out, ev in ((Ht, evh), (f["G"], f["dft"])):                      # both transforms
        assert ev["v_identity"] == _TOTAL and len(set(out)) == 1 and out[0] != 0             # one point repeated
    # every G'_j is that point: the terms of a wire double (coefficients 1, 1) and cancel (1, r - 1), in the level over the
    # terms and above, and runs that sum to the identity go up as pieces
    e = f["ev"]
    assert e["equal@0"] >= 20 and e["opposite@0"] >= 20 and e["piece_identity@0"] >= 10 and e["piece_identity@up"] >= 1
    assert e["add_identity@up"] >= 20 and e["term_g_identity"] == 0
    Ht, evh, f = dk.case_events("index_half")
    for out, ev in ((Ht, evh), (f["G"], f["dft"])):
        assert ev["u_identity_v_finite"] == 1 and ev["v_identity"] == _TOTAL - 1
        assert out[0] != 0 and all(out[j] == (out[0] if j % 2 == 0 else R - out[0]) for j in range(64))    # P, -P, P, ...
    assert f["ev"]["equal@0"] >= 10 and f["ev"]["opposite@0"] >= 5


@pytest.mark.parametrize("name", ["geometric_low/h", "geometric_high/fold"])
def test_geometric_family(name):
    """an odd exponent: opposite at k = 0 in the first stage, then equal and opposite after a twiddle multiplication"""
    out, ev, f = _aimed(name)
    assert ev["u_eq_neg_t_k0"] == 31 and ev["u_eq_t_k"] >= 7 and ev["u_eq_neg_t_k"] >= 15 and ev["u_identity_v_finite"] == 57


def test_every_second_family():
    Ht, evh, f = dk.case_events("every_second")
    for out, ev in ((Ht, evh), (f["G"], f["dft"])):
        assert ev["v_identity"] == 112 and ev["generic"] == 80 and out[:32] == out[32:] and 0 not in out       # period n/2


@pytest.mark.parametrize("name", ["half_period/h", "half_period/fold"])
def test_half_period_family(name):
    out, ev, f = _aimed(name)
    assert ev["u_eq_t_k0"] == 31 and ev["identity_outputs"] == 32 and all(out[j] == 0 for j in range(1, 64, 2))
    if name.endswith("fold"):
        assert f["ev"]["term_g_identity"] >= 60 and f["ev"]["instance_p_identity"] == 1


@pytest.mark.parametrize("name", ["pair/h", "pair/fold"])
def test_pair_family(name):
    out, ev, f = _aimed(name)
    assert ev["u_eq_t_k0"] == 1 and ev["u_eq_neg_t_k0"] == 1 and ev["u_eq_neg_t_k"] + ev["u_eq_t_k"] == 1      # the last: output 5
    assert ev["identity_outputs"] == 1 and out[5] == 0 and ev["u_identity_v_finite"] == 2 and ev["generic"] == 186
    if name.endswith("fold"):
        assert f["ev"]["term_g_identity"] >= 1


@pytest.mark.parametrize("name", ["two_tone/h", "two_tone/fold"])
def test_two_tone_family(name):
    out, ev, f = _aimed(name)
    assert ev["identity_outputs"] == 62 and out[3] and out[59] and ev["u_eq_neg_t_k"] >= 10 and ev["u_eq_t_k"] >= 10
    if name.endswith("fold"):
        e = f["ev"]
        assert e["term_g_identity"] >= 130 and e["piece_identity@0"] >= 20 and e["piece_identity@up"] >= 5 and e["instance_p_identity"] == 2
        assert sum(1 for v in f["folded"] if v == 0) >= 26 and e["fold_both_identity"] >= 20       # 30 bases, nearly all the identity


@pytest.mark.parametrize("name", [n for n in dk.CASES if n != "two_tone/fold" and not n.startswith("D")])
def test_what_the_matrices_give_every_key(name):
    """coefficients 0 and 1 among the terms, the hot column's run over more than two levels, a finite P_k on an instance wire with
    identity l points elsewhere, the wire absent from C"""
    circ, _, _ = dk.case_key(name)
    e = dk.case_events(name)[2]["ev"]
    assert e["levels"] >= 3 and e["term_g_identity"] + e["term_coeff_zero"] + e["term_coeff_one"] + e["term_other"] == sum(map(len, circ.mats[2]))
    assert e["term_coeff_zero"] >= 1 and e["term_coeff_one"] >= 1 and e["instance_p_finite"] >= 1
    assert e["fold_p_identity_l_finite"] >= 1 and e["fold_l_identity_p_finite"] + e["fold_both_identity"] >= 1


def test_aimed_l_query():
    circ, key, roles = dk.case_key("aimed_l")
    _, evh, f = dk.case_events("aimed_l")
    e = f["ev"]
    assert e["fold_p_eq_l"] == 1 and e["fold_p_eq_neg_l"] == 1 and e["fold_both_identity"] == 1
    assert e["fold_l_identity_p_finite"] >= 1 and e["fold_p_identity_l_finite"] >= 1 and e["instance_p_finite"] == 2
    assert f["folded"][roles["cancelling"]] == 0 and f["folded"][roles["doubling"]] == 2 * f["P"][roles["doubling"]] % R
    assert f["folded"][roles["both_identity"]] == 0 and f["P"][roles["p_identity"]] == 0 and f["folded"][roles["p_identity"]] != 0
    assert f["dft"]["generic"] == 191 and evh["generic"] == 191           # the transforms themselves are the generic ones


def test_small_and_large_domains():
    """D = 2 (one butterfly, its V the missing point), D = 4 and D = 1024 (a stage of 512 butterflies: two workgroups)"""
    out, ev, f = _aimed("D2/index0")
    assert ev["v_identity"] == 1 and out[0] == out[1] != 0
    assert f["ev"]["opposite@0"] >= 30 and f["ev"]["levels"] == 3            # one row holds the whole hot column
    out, ev, f = _aimed("D4/constant")
    assert ev["u_eq_t_k0"] == 1 and ev["v_identity"] == 1 and ev["u_identity_v_finite"] == 1 and ev["generic"] == 1
    for name in ("D1024/two_tone/h", "D1024/two_tone/fold"):
        out, ev, f = _aimed(name)
        assert ev["identity_outputs"] == 1022 and ev["u_eq_neg_t_k"] >= 150 and ev["u_eq_t_k"] >= 150 and ev["u_eq_neg_t_k0"] >= 400
        assert sum(ev[e] for e in dk.DFT_EVENTS) == 512 * 10
