"""cg_device_link_prove_batch behind cg_create_showings_batch: the openings of the two device key values are cut out of the
arrays the showing call took (Groth16.device_link_openings, the rule of csrc/show_make.hpp's mk_link_opening), the device proofs
are made on that call's own `committed`, and both verifying calls accept all of it.

This case of tests/test_gpu_device_link_make.py lives in a file of its own, which runs later, for the reason
tests/test_gpu_showings_device_link.py states: the showing calls' pairing kernels declare a private segment, and
tests/test_gpu_fullsize.py must find the device's memory as the runtime left it."""
import random
from types import SimpleNamespace

import numpy as np
import pytest

import device_link_vectors as D
import test_gpu_showings_create as C
import test_gpu_showings_whole as W

pytestmark = pytest.mark.gpu

R = D.R
MADE, ACCEPT = 1, D.ACCEPT


@pytest.fixture(scope="module")
def world(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()
    w = W.World(cc, "mdl", 4, 0xD11C)
    yield w
    w.close()


def test_device_proofs_from_whole_showings(world):
    w, G = world, world.cc.Groth16
    n, rng = 4, random.Random(0x5401)
    pos0, pos1 = w.com                                            # the mDL-like layout's two committed inputs as the device key values
    b = C.states(w, n, distinct=4)
    res = C.one_call(b)
    assert res["status"].tolist() == [MADE] * n
    proofs, inputs, rand, _, _ = b.packed()
    openings = G.device_link_openings(w.io, pos0, pos1, inputs, rand)
    for i in range(n):                                            # the rule, stated once more on this batch's own values
        want = [b.xs[i][pos0], b.rows[i][2 + 0], b.xs[i][pos1], b.rows[i][2 + 1]]
        assert openings[i].tobytes() == b"".join(D.fe(v) for v in want)
    dl_rand = b"".join(D.fe(rng.randrange(R)) for _ in range(9 * n))
    h_q = bytes(rng.randrange(256) for _ in range(32 * n))
    com1, comz, m, c0, s0, c1, s1, e, status = G.device_link_prove_batch_packed(w.pvk, w.io, pos0, pos1, res["committed"], openings, dl_rand, h_q)
    assert status.tolist() == [MADE] * n
    # the showings verify, and so do their device proofs, on the same `committed`
    verdicts, parts = w.verify(C.recs_of(b, res))
    assert verdicts.tolist() == [ACCEPT] * n and parts.tolist() == [[ACCEPT] * (1 + len(w.com))] * n
    verdicts, parts, e_v = G.device_link_verify_batch_packed(w.pvk, w.io, pos0, pos1, res["committed"], com1, comz, h_q, m, c0, s0, c1, s1)
    assert verdicts.tolist() == [ACCEPT] * n and parts.tolist() == [[ACCEPT, ACCEPT]] * n
    assert e_v.tobytes() == e.tobytes()
    # and by the restatement, which reads the same bytes
    gabc = w.vk["gamma_abc_g1"]
    key = SimpleNamespace(g=gabc[pos0 + 1], gp=gabc[pos1 + 1], h=w.vk["delta_g1"], ci0=0, ci1=1)
    for i in range(n):
        row = (res["committed"][i].tobytes(), com1[i].tobytes(), comz[i].tobytes(), h_q[32 * i:32 * i + 32], m[i].tobytes(), c0[i].tobytes(),
               s0[i].tobytes(), c1[i].tobytes(), s1[i].tobytes())
        assert D.verify(key, row) == (ACCEPT, (ACCEPT, ACCEPT), e[i].tobytes()), i
    # an opening of a neighbour's showing does not open this one's committed points
    swapped = openings[[1, 0, 2, 3]].copy()
    status = G.device_link_prove_batch_packed(w.pvk, w.io, pos0, pos1, res["committed"], swapped, dl_rand, h_q)[8]
    assert status.tolist() == [2, 2, MADE, MADE]
