"""cg_device_link_verify_batch after a cg_verify_showings_batch on the same cg_pvk: the two entries share the handle, its
stream and its lock, and each has its own per-call arrays, so the device link answers with the same bytes before and after.

This case of tests/test_gpu_device_link.py lives in a file of its own, which runs later: the verifier's pairing kernels declare
a private segment, the runtime keeps that memory for the rest of the process, and tests/test_gpu_fullsize.py - between the two
files - fills the device's memory to a stated remainder and must find it as the runtime left it."""
import pytest

import test_gpu_device_link as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mdl(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()
    w = T.World(cc, "mdl", 0x3D1)
    yield w
    w.pvk.close()


def test_the_same_bytes_after_a_showing_call_on_the_handle(mdl):
    cc, k = mdl.cc, mdl.key
    rows = [mdl.row(r) for r in mdl.recs[:5]] + [mdl.row(T.but(mdl.recs[5], m=T.R))]
    flat = lambda res: [a.tobytes() for a in res]
    first = flat(mdl.call(rows))
    assert [int(v) for v in mdl.call(rows)[0]] == [T.ACCEPT] * 5 + [T.MALFORMED]
    n_rev, n_hid, n_com = (k.io.count(t) for t in (T.REV, T.HID, T.COM))
    # one showing of zero bytes: malformed, and every kernel of the entry runs on the handle's stream
    verdicts, _ = cc.Groth16.verify_showings_batch_packed(mdl.pvk, None, k.io, bytes(32 * n_rev), bytes(256), bytes(64), bytes(64 * n_com), bytes(32),
                                                          bytes(32 * (2 * n_com + n_hid + 1)), [], b"", [], context=b"ctx")
    assert len(verdicts) == 1 and int(verdicts[0]) != T.ACCEPT
    assert flat(mdl.call(rows)) == first
    for i, row in enumerate(rows):
        v, p, d = mdl.want(row)
        assert (first[0][i], tuple(first[1][2 * i:2 * i + 2]), first[2][32 * i:32 * i + 32]) == (v, p, d), i
