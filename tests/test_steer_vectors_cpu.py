"""tests/steer_vectors.py against its own integer model: every steered vector hits the case it is named for - a condition,
not a statistic -, every family has the stated number of vectors, and every expected status comes from the oracles
(tests/p256_vectors.py, tests/poseidon_vectors.py).  A search that runs out raises, so nothing is skipped.  Pure CPU."""
import random

import p256_vectors as V
import poseidon_vectors as PV
import steer_vectors as S

P, N, R = S.P, S.N, S.R
MADE, MALFORMED, BAD_SIGNATURE = V.MADE, V.MALFORMED, V.BAD_SIGNATURE
num = lambda b: int.from_bytes(b, "big")


def by_words(a, b, m, bits):
    """a word-by-word Montgomery product before its last conditional subtraction, as csrc/fq256.hpp runs it"""
    w = 1 << bits
    minv = -pow(m, -1, w) % w
    t = 0
    for i in range(256 // bits):
        t += a * ((b >> (bits * i)) & (w - 1))
        t += (t * minv % w) * m
        assert t % w == 0
        t >>= bits
    return t


def test_the_model_is_the_word_by_word_product_for_both_word_sizes_and_both_moduli():
    rng = random.Random(0x30DE1)
    for m in (P, N):
        pairs = [(m - 1, m - 1), (0, 0), (1, 1), (m - 1, 1), (R * R % m, m - 1)] + [(rng.randrange(m), rng.randrange(m)) for _ in range(200)]
        small = [S.unmont(rng.randrange(1, 1 << 200), m) for _ in range(50)]
        pairs += [(x, R * R % m) for x in small]
        for a, b in pairs:
            want = S.pre(a, b, m)
            assert by_words(a, b, m, 32) == by_words(a, b, m, 64) == want < 2 * m
            assert want % m == a * b * pow(R, -1, m) % m
        assert all(S.from_words_hits(x, m) for x in small)
        assert not any(S.mul_hits(rng.randrange(m), rng.randrange(m), m) for _ in range(200))       # 2^-32 each
    assert S.rare(P, P) and S.rare(R - 1, P) and not S.rare(P - 1, P) and not S.rare(R, P)
    assert S.DELTA_MAX == 2**224 - 2**192 - 2**96 and (P - 1) % 25 == 0 and (P - 1) % 125 != 0 and pow(S.W25, 5, P) != 1 == pow(S.W25, 25, P)
    assert all(pow(S.fifth_root(pow(x, 5, P)), 5, P) == pow(x, 5, P) and S.is_fifth_power(pow(x, 5, P)) for x in range(2, 60))
    assert sum(S.is_fifth_power(x) for x in range(2, 502)) < 150


def test_both_constructions_make_valid_rows_with_the_stated_scalars():
    rng = random.Random(0x30DE2)
    X, Q = S.rand_point(rng), S.rand_point(rng)
    for u, v in ((0x77, 0x99), (0, 5), (1, 1), (N - 1, N - 1), (rng.randrange(N), rng.randrange(1, N))):
        row = S.forged_r(X, u, v)
        st, r_xy, _, _ = V.compute_rtu(*row)
        assert st == MADE and r_xy == V.point_bytes(X)
        r = X[0] % N
        assert S.rtu_scalars(*row) == [v, v * pow(r, -1, N) % N, u, u * pow(r, -1, N) % N, -num(row[2]) * pow(r, -1, N) % N]
        if v > 1 or u > 1:
            row = S.free_q(Q, u, v)
            assert V.compute_rtu(*row)[0] == MADE and row[0] == V.point_bytes(Q) and S.rtu_scalars(*row)[0] == v and S.rtu_scalars(*row)[2] == u
    y = S.unmont(12345, P)
    while S.x_of_y(y) is None:
        y = S.unmont(S.mont(y, P) + 1, P)
    assert V.on_curve((S.x_of_y(y), y))


def test_family_counts():
    fam = S.p256_families()
    assert {k: len(v) for k, v in fam.items()} == S.P256_COUNTS
    assert sum(S.P256_COUNTS.values()) == 52 + 12 + 28 + 30
    names = [v.name for vs in fam.values() for v in vs]
    assert len(set(names)) == len(names)
    pos = S.poseidon_families()
    assert dict({k: len(v) for k, v in pos.items()}, hq=len(S.hq_vectors())) == S.POSEIDON_COUNTS


def test_rx_above_n_rows_hold_an_x_in_n_to_p_and_the_oracle_gives_each_status():
    vecs = S.p256_families()["rx_above_n"]
    assert sorted({S.facts(v)["X"][0] - N for v in vecs}) == [3, 4, 6, 9]
    seen = {MADE: 0, MALFORMED: 0, BAD_SIGNATURE: 0}
    for v in vecs:
        f, want = S.facts(v), S.expected(v)
        X = f["X"]
        assert N <= X[0] < P and V.on_curve(X), v.name
        assert want[0] == v.status, v.name
        seen[v.status] += 1
        if v.kind == "tu":
            assert v.args[0] == V.point_bytes(X) and want[1] != V.ZERO_POINT
        elif v.status == MADE:
            assert want[1] == V.point_bytes(X) and num(v.args[1][:32]) == X[0] - N
            sc = S.rtu_scalars(*v.args)
            assert (sc[2], sc[0]) == (f["u"], f["v"])
        elif v.status == MALFORMED:
            assert num(v.args[1][:32]) == X[0] and want[1:] == (V.ZERO_POINT,) * 3
        else:
            assert num(v.args[1][:32]) == X[0] - N + 1 and want[1:] == (V.ZERO_POINT,) * 3
    assert seen == {MADE: 20, MALFORMED: 16, BAD_SIGNATURE: 16}
    assert {(S.facts(v).get("u"), S.facts(v).get("v")) for v in vecs if v.kind == "rtu" and v.status == MADE} == {(0x77, 0x99), (0, 5), (1, 1), (N - 1, N - 1)}


def test_digest_rows_are_zero_or_not_below_n_and_u_is_the_identity_where_it_must_be():
    vecs = S.p256_families()["digests"]
    assert sorted(S.facts(v)["digest"] for v in vecs if v.kind == "rtu") == [0, 0, N, N, N + 5, R - 1]
    for rtu, tu in zip(vecs[0::2], vecs[1::2]):
        assert (rtu.kind, tu.kind) == ("rtu", "tu") and rtu.args[2] == tu.args[1]
        d = num(rtu.args[2])
        assert d == S.facts(rtu)["digest"] and (d % N == 0 or d >= N)
        st, r_xy, t, u = S.expected(rtu)
        assert st == MADE and tu.args[0] == r_xy and S.expected(tu) == (MADE, t, u), rtu.name
        assert (u == V.ZERO_POINT) == (d % N == 0) and t != V.ZERO_POINT and r_xy != V.ZERO_POINT
        sc = S.rtu_scalars(*rtu.args)
        assert (sc[2:] == [0, 0, 0]) == (d % N == 0)
    assert [S.rtu_scalars(*v.args)[2] for v in vecs[0:12:2]].count(0) == 4


def test_structured_scalar_rows_carry_the_named_scalar_in_the_named_term():
    vecs = S.p256_families()["structured_scalars"]
    walks = [v for v in vecs if v.kind == "tu"]
    chains = [v for v in vecs if v.kind == "rtu"]
    assert [S.facts(v)["scalar"] for v in walks] == list(S.WALK_SCALARS) and len(S.WALK_SCALARS) == 10
    assert 1 in S.WALK_SCALARS and N - 1 in S.WALK_SCALARS and 255 << 248 in S.WALK_SCALARS and S.ZERO_WINDOWS in S.WALK_SCALARS and S.ONES in S.WALK_SCALARS
    for v in walks:
        k = S.facts(v)["scalar"]
        assert S.facts(v)["term"] == 1 and S.tu_scalars(*v.args)[1] == k, v.name
        st, t, u = S.expected(v)
        assert st == MADE and u == V.point_bytes(V.mul(k, V.G)), v.name
    for term in (0, 1):
        assert [S.facts(v)["scalar"] for v in chains if S.facts(v)["term"] == term] == list(S.CHAIN_SCALARS)
    assert len(S.CHAIN_SCALARS) == 9 and {1, 15, 16, 17, 1 << 252, 15 << 252, N - 1, S.ZERO_WINDOWS % N} <= set(S.CHAIN_SCALARS)
    for v in chains:
        f = S.facts(v)
        assert S.rtu_scalars(*v.args)[f["term"]] == f["scalar"] and S.expected(v)[0] == MADE, v.name
    # what "mostly zero" means for the two window sizes
    assert sum(((S.ZERO_WINDOWS >> (8 * w)) & 255) == 0 for w in range(32)) == 29
    assert sum(((S.ZERO_WINDOWS >> (4 * w)) & 15) == 0 for w in range(64)) == 60


def test_entry_point_rows_hit_their_site():
    vecs = S.p256_families()["entry_points"]
    sites = {}
    for v in vecs:
        f = S.facts(v)
        sites[f["site"]] = sites.get(f["site"], 0) + 1
        assert S.expected(v)[0] == MADE == v.status, v.name
        if "point" in f:
            pt = f["point"]
            assert V.on_curve(pt) and v.args[0] == V.point_bytes(pt) and f["site"] in S.coordinate_sites(pt), v.name
        elif f["site"] == "d":
            d = num(v.args[-1])
            assert d == f["scalar"] < N and S.reduced_from_words_hits(d, N), v.name
        elif f["site"] == "s":
            assert num(v.args[1][32:]) == f["scalar"] and S.from_words_hits(f["scalar"], N), v.name
        else:
            assert f["site"] == "r" and f["scalar"] < N and S.reduced_from_words_hits(f["scalar"], N), v.name
            assert num(v.args[1][:32] if v.kind == "rtu" else v.args[0][:32]) == f["scalar"]
            if v.kind == "rtu":
                assert num(S.expected(v)[1][:32]) == f["scalar"]
    assert sites == {"x from_words": 4, "y from_words": 4, "x + x": 4, "2x + x, 2m < p": 4, "2x + x, 2m >= p": 4, "d": 4, "s": 2, "r": 4}
    # the sites in words: 2m in [p, 2^256); 3m in [p, 2^256); 3m - p in [p, 2^256) after 2m passed 2^256
    for v in vecs:
        f = S.facts(v)
        if "point" in f:
            m = S.mont(f["point"][0], P)
            if f["site"] == "x + x":
                assert P <= 2 * m < R
            elif f["site"] == "2x + x, 2m < p":
                assert 2 * m < P <= 3 * m < R
            elif f["site"] == "2x + x, 2m >= p":
                assert 2 * m >= R and P <= 3 * m - P < R
            elif f["site"] == "x from_words":
                assert P <= S.pre(f["point"][0], R * R % P, P) < R
            else:
                assert P <= S.pre(f["point"][1], R * R % P, P) < R


def test_every_site_of_round_0_is_hit_by_its_own_state():
    c = PV.p256()
    all_sites = set(S.round0_sites((1, 2, 3)))
    assert len(all_sites) == 3 + 9 + 9 + 6
    covered = set()
    for name, vecs in S.poseidon_families().items():
        for v in vecs:
            assert all(0 <= x < P for x in v.state) and len(v.state) == 3
            value = S.round0_sites(v.state)[v.site]
            assert P <= value < R, v.name
            assert v.site[0] == name or (name == "pow5" and v.site[0] in ("sqr", "sqr_sqr", "mul_a4_a"))
            covered.add(v.site)
    # six of the matrix's nine products cannot take the branch on any input (steer_vectors.mds_mul_reachable has the proof)
    never = {("mds_mul", 3 * i + j) for i in range(3) for j in range(3) if not S.mds_mul_reachable(i, j)}
    assert never == {("mds_mul", e) for e in (0, 1, 2, 3, 4, 6)}
    assert covered == all_sites - never and not covered & never
    rng = random.Random(0x30DE3)
    for _, e in sorted(never):
        a, k = S.mont(c.mds[e // 3][e % 3], P), e // 3 + e % 3 + 3
        ts = [0, 1, S.DELTA_MAX, S.DELTA_MAX - 1] + [rng.randrange(S.DELTA_MAX + 1) for _ in range(200)]
        assert not any(S.mul_hits(a, t * k, P) for t in ts)              # the only operands that could
    adds = S.poseidon_families()["add_rc"]
    assert sorted(S.round0_sites(v.state)[v.site] - P for v in adds) == sorted([0, 1, S.DELTA_MAX] * 3)
    assert max(S.round0_sites(v.state)[v.site] for v in adds) == R - 1
    # the model's round 0 is the oracle's: one round by hand
    st = adds[0].state
    post = [pow((x + k) % P, 5, P) for x, k in zip(st, c.rc[:3])]
    assert all(S.round0_sites(st)[("mds_mul", 3 * i + j)] % P == S.mont(c.mds[i][j] * post[j], P) for i in range(3) for j in range(3))


def test_hq_triples_are_scalars_of_bn254_and_hit_their_sites():
    vecs = S.hq_vectors()
    assert [v.sites for v in vecs] == [("q0",), ("q1",), ("q0", "q1"), ("z",), ("z",), ("q0", "q1", "z")]
    for v in vecs:
        assert all(0 <= x < S.FR for x in v.q)
        assert set(v.sites) <= S.hq_sites(*v.q), v.name
