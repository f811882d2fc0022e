"""tests/p256_vectors.py, the oracle of the P-256 tests, against what is known without it: the NIST P-256 / SHA-256 example the
reference tests with (tests/golden/p256_ecdsa_kats.json), the two identities that make T and U the public inputs of the
modified verification equation - s T + U = Q and r T = R - on seeded signatures, and every status path of the two
restatements.  Pure CPU, no build."""
import pytest

from conftest import load_golden
import p256_vectors as V

K = load_golden("p256_ecdsa_kats.json")
N, P, G = V.N, V.P, V.G
val = lambda name: int(K[name], 16)
as_point = lambda b: None if b == V.ZERO_POINT else (int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big"))


def kat_row():
    return V.point_bytes((val("q_x"), val("q_y"))), V.be(val("r")) + V.be(val("s")), bytes.fromhex(K["digest"])


def test_the_curve_and_the_example_key():
    assert V.on_curve(G) and V.mul(N, G) is None and V.mul(N - 1, G) == V.neg(G)
    assert V.mul(val("private_key"), G) == (val("q_x"), val("q_y"))


def test_the_nist_example_through_both_restatements():
    q, sig, dg = kat_row()
    status, r_xy, t_xy, u_xy = V.compute_rtu(q, sig, dg)
    assert status == V.MADE
    assert r_xy == V.be(val("r")) + V.be(val("r_y"))                  # the signature verifies, and R.y is the recorded one
    assert K["r_y"].startswith("3ce76603") and K["r_y"].endswith("8174b5")
    T, U = as_point(t_xy), as_point(u_xy)
    assert V.add(V.mul(val("s"), T), U) == (val("q_x"), val("q_y"))   # the modified verification equation
    assert V.compute_tu(r_xy, dg) == (V.MADE, t_xy, u_xy)
    # the signer reproduces the example from its nonce, k = (d + r priv) / s
    k = (int(K["digest"], 16) + val("r") * val("private_key")) * pow(val("s"), -1, N) % N
    assert V.sign(val("private_key"), dg, k) == ((val("q_x"), val("q_y")), val("r"), val("s"))


def test_t_and_u_satisfy_the_modified_equation_on_32_seeded_signatures():
    for q, sig, dg in V.signed_rows(0x5EED, 32):
        status, r_xy, t_xy, u_xy = V.compute_rtu(q, sig, dg)
        assert status == V.MADE
        R, T, U, Q = as_point(r_xy), as_point(t_xy), as_point(u_xy), as_point(q)
        r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
        assert V.add(V.mul(s, T), U) == Q and V.mul(r, T) == R and R[0] % N == r
        assert V.compute_tu(r_xy, dg) == (V.MADE, t_xy, u_xy)


def test_every_status_path():
    q, sig, dg = V.signed_rows(0x57A7, 1)[0]
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    _, r_xy, t_xy, u_xy = V.compute_rtu(q, sig, dg)
    zero3 = (V.ZERO_POINT,) * 3
    x, y = as_point(r_xy)
    # compute_TU
    for bad in (V.be(P) + r_xy[32:], V.be((1 << 256) - 1) + r_xy[32:], r_xy[:32] + V.be(P), r_xy[:32] + V.be(y + 1), V.be(x + 1) + r_xy[32:]):
        assert V.compute_tu(bad, dg) == (V.MALFORMED, V.ZERO_POINT, V.ZERO_POINT)
    status, t0, u0 = V.compute_tu(r_xy, bytes(32))
    assert (status, u0) == (V.MADE, V.ZERO_POINT) and t0 == t_xy          # d = 0: U is the identity, T does not depend on d
    assert V.compute_tu(r_xy, V.be(N)) == (V.MADE, t0, u0)                # a digest >= n is reduced
    d5 = V.compute_tu(r_xy, V.be(N + 5))
    assert d5 == V.compute_tu(r_xy, V.be(5)) and d5[0] == V.MADE and d5[2] != V.ZERO_POINT
    # compute_RTU
    qx, qy = as_point(q)
    for bad_q in (V.be(P) + q[32:], q[:32] + V.be(qy + 1)):
        assert V.compute_rtu(bad_q, sig, dg) == (V.MALFORMED,) + zero3
    for bad_sig in (V.be(0) + sig[32:], V.be(N) + sig[32:], sig[:32] + V.be(0), sig[:32] + V.be(N), V.be((1 << 256) - 1) + sig[32:]):
        assert V.compute_rtu(q, bad_sig, dg) == (V.MALFORMED,) + zero3
    assert V.compute_rtu(q, V.be(r - 1) + sig[32:], dg) == (V.BAD_SIGNATURE,) + zero3
    assert V.compute_rtu(q, sig, V.be(int.from_bytes(dg, "big") ^ 1)) == (V.BAD_SIGNATURE,) + zero3
    # (r, n - s) is the other valid signature of the same digest: R' = -R has the same x
    status, r2, _, _ = V.compute_rtu(q, sig[:32] + V.be(N - s), dg)
    assert status == V.MADE and as_point(r2) == V.neg(as_point(r_xy))


@pytest.mark.parametrize("priv", [1, N - 1, 0x1234567])
def test_the_rows_a_signer_can_arrange(priv):
    """Q = G, Q = -G, and the two coincidences of the partial sums: each row hits its case"""
    row = V.coincident_row(priv, 0xC0FFEE)
    uG, vQ = V.terms_of(*row)
    assert uG == vQ and V.compute_rtu(*row)[0] == V.MADE
    assert as_point(V.compute_rtu(*row)[1]) == V.add(uG, uG)
    row = V.coincident_row(priv, 0xC0FFEE, opposite=True)
    uG, vQ = V.terms_of(*row)
    assert uG == V.neg(vQ) and uG is not None and V.compute_rtu(*row) == (V.BAD_SIGNATURE,) + (V.ZERO_POINT,) * 3
    assert as_point(V.coincident_row(1, 5)[0]) == G and as_point(V.coincident_row(N - 1, 5)[0]) == V.neg(G)
