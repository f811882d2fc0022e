"""The two-call Groth16 showing paths finished by the library's Merlin (cg_dlog_challenge_batch through
Groth16.show_batch(challenge=None) and Groth16.verify_show_batch(context=...)): the challenge of every showing equals
`DLogPoK`'s transcript as tests/merlin_vectors.py computes it from the key's own points - per committed input the statement
(gamma_abc_g1[i + 1], delta_g1), then the hidden inputs' bases and delta_g1 (creds/src/groth16rand.rs:133-174, :246-300) -
and the verifier accepts exactly the showings whose context and challenge match."""
import random

import pytest

import bn254_oracle as o
import merlin_vectors as MV
import show_create_vectors as M
import show_vectors as S
import verify_vectors as V

pytestmark = pytest.mark.gpu

cmp = o.g1_compressed
ACCEPT = 1


@pytest.fixture(scope="module", autouse=True)
def _init(cc):
    rc = cc.lib().cg_init(0, None)
    assert rc == 0, cc.lib().cg_last_error()


def compress(b):
    from crescent_credentials_amd import api
    return api._g1_compress(b).tobytes()


def want_challenge(vk, io, k, sg, context):
    abc, delta = vk["gamma_abc_g1"], cmp(vk["delta_g1"])
    com = [i for i, t in enumerate(io) if t == S.COMMITTED]
    hid = [j for j, t in enumerate(io) if t == S.HIDDEN]
    st = [([cmp(abc[i + 1]), delta], k[n].tobytes(), compress(sg.commited_inputs[n])) for n, i in enumerate(com)]
    st.append(([cmp(abc[j + 1]) for j in hid] + [delta], k[len(com)].tobytes(), compress(sg.com_hidden_inputs)))
    return MV.to_int(MV.dlog_challenge(context, st))


@pytest.mark.parametrize("layout", ["mixed", "hidden", "committed"])
def test_showings_made_and_verified_with_the_librarys_merlin(cc, layout):
    rng, sc, vk, xs, abc = M.synthetic(6, 0x717)
    io = M.layout(layout, 6)
    made = [M.make(vk, M.proof_of(abc), xs, io, rng) for _ in range(3)]
    states = [(m.proof_bytes, m.inputs) for m in made]
    revealed = [x for x, t in zip(xs, io) if t == S.REVEALED]
    context = b"presentation"
    with cc.PreparedVerifyingKey(cc.Groth16.prepare_verifying_key(V.vk_bytes(vk))) as gpu:
        assert gpu.delta_g1.tobytes() == o.g1_uncompressed(vk["delta_g1"])
        assert gpu.gamma_abc_g1.tobytes() == b"".join(o.g1_uncompressed(P) for P in vk["gamma_abc_g1"])
        shows = cc.Groth16.show_batch(gpu, io, states, context=context)
        pairs = [(sg, revealed) for sg in shows]
        verdicts, k = cc.Groth16.verify_show_batch(gpu, io, pairs)
        assert list(verdicts) == [ACCEPT] * 3
        for i, sg in enumerate(shows):
            assert sg.pok_c == want_challenge(vk, io, k[i], sg, context), i
            assert sg.pok_c < 1 << 248
        assert cc.Groth16.verify_show_batch(gpu, io, pairs, context=context) == [True] * 3
        assert cc.Groth16.verify_show_batch(gpu, io, pairs, context=b"presentatioN") == [False] * 3
        assert cc.Groth16.verify_show_batch(gpu, io, pairs, context=None) == [False] * 3
        none = cc.Groth16.show_batch(gpu, io, states[:1])                        # the reference's context None
        assert none[0].pok_c == want_challenge(vk, io, cc.Groth16.verify_show_batch(gpu, io, [(none[0], revealed)])[1][0], none[0], None)
        assert cc.Groth16.verify_show_batch(gpu, io, [(none[0], revealed)], context=None) == [True]
        assert cc.Groth16.verify_show_batch(gpu, io, [(none[0], revealed)], context=b"") == [True]          # None is the empty string
        # a spoiled showing between two good ones
        bad = cc.ShowGroth16(shows[1].rand_proof, shows[1].com_hidden_inputs, shows[1].pok_c ^ 1, shows[1].pok_s, shows[1].commited_inputs)
        assert cc.Groth16.verify_show_batch(gpu, io, [pairs[0], (bad, revealed), pairs[2]], context=context) == [True, False, True]
        assert cc.Groth16.verify_show_batch(gpu, io, [], context=context) == []
        # a callable behaves as before
        c = rng.randrange(1 << 248)
        assert [sg.pok_c for sg in cc.Groth16.show_batch(gpu, io, states, lambda *a: c)] == [c] * 3
