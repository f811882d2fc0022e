"""tests/poseidon_vectors.py against the values the reference records about its own Poseidon (tests/golden/neptune_kats.json,
all over BLS12-381's Fr), and then its P-256 instantiation against itself.  What the recorded values pin: the round numbers,
the Grain LFSR at 255 bits, the Cauchy matrix, the plain round function, the IO-pattern tag.  What they do not:
poseidon_vectors' three readings.  Pure CPU, Python integers only."""
import json
import os

import pytest

from conftest import ROOT
import poseidon_vectors as PV

K = json.load(open(os.path.join(ROOT, "tests", "golden", "neptune_kats.json")))
BLS = int(K["bls12_381_fr"], 16)


@pytest.fixture(scope="module")
def bls3():
    return PV.Constants(BLS, K["bls12_381_fr_bits"], 3)


def test_modulus_constants():
    assert BLS == PV.BLS12_381_FR and BLS.bit_length() == 255
    assert PV.P256.bit_length() == 256 and PV.P256 % (1 << 96) == (1 << 96) - 1
    assert PV.BN254_FR < PV.P256


def test_round_numbers_equal_the_recorded_rows():
    for t, want in K["round_numbers"].items():
        if t.startswith("_"):
            continue
        assert list(PV.round_numbers(int(t))) == want, t


def test_arity_2_standard_digest(bls3):
    k = K["arity2_standard"]
    assert (bls3.rf, bls3.rp) == (8, 55)
    out = PV.permute(bls3, [k["domain_tag"]] + k["preimage"])
    assert "%064x" % out[1] == k["digest"]
    assert k["digest"].endswith("2e203c369a02e7ff")


def test_tag_values():
    non_trivial = 0
    for row in K["tag_values"]:
        assert PV.io_tag([tuple(x) for x in row["pattern"]], row["domain_separator"]) == int(row["value"])
        non_trivial += int(row["value"]) != 0
    assert non_trivial >= 3


def test_first_round_constants_of_width_9():
    k = K["round_constants_t9"]
    c = PV.Constants(BLS, k["field_bits"], k["t"])
    assert (c.rf, c.rp, len(c.rc)) == (k["r_f"], k["r_p"], k["count"])
    assert ["%064x" % x for x in c.rc[:3]] == k["first"]
    assert PV.first_byte_bits(k["field_bits"]) == 7 and PV.first_byte_bits(256) == 8


# ---- the P-256 instantiation against itself ---------------------------------------------------------------------------------
def test_p256_constants():
    c, p = PV.p256(), PV.P256
    assert (c.rf, c.rp) == (8, 55) and len(c.rc) == 189 and all(0 <= x < p for x in c.rc)
    assert len(set(c.rc)) == 189
    m = c.mds
    assert all(m[i][j] == m[j][i] for i in range(3) for j in range(3))
    assert all(m[i][j] * (i + j + 3) % p == 1 for i in range(3) for j in range(3))
    det = (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
           + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0])) % p
    assert det != 0
    assert len(PV.table()) == 199


def test_p256_vector():
    assert PV.HQ_TAG == 0xffffffffffffffffffffffb0800060e4
    assert PV.hq(1, 2, 3).hex() == "b4c83f5ebbc2a8a6c913d1361168ceee2d3796453258470cb7ac7c3abeb24ab5"
    assert PV.hq_bytes(1) == bytes(31) + b"\x01"
