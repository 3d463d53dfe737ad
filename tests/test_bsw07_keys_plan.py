"""BSW07 decryption with a key per item through the host planner (gopairingbasedcryptography_amd/bsw07.py: leaf_mask, used_columns,
decrypt_batch_keys) on the oracle stand-in engine (tests/bsw07_keys_fixture.py; the same flow runs on the GPU engine in
test_bsw07_keys_gpu.py): the messages of the fixture come back for the users whose attributes satisfy the policy, the others get ok = 0
and a zero row, and the lists that reach multi_pair hold the used leaves only, in leaf order, padded with points at infinity."""
import numpy as np
import pytest

from bsw07_fixture import Instance, example_tree
from bsw07_keys_fixture import GARBAGE, ciphertext_arrays, user_keys
from standin_engine import StandInEngine, TensorEngine, recorded, same_on_tensors, tensors
from gopairingbasedcryptography_amd import bsw07

L, T = bsw07.Leaf, bsw07.Threshold
# the example tree: 2 of (11, 2 of (22, 33), 44, 1 of (55, 11)); leaf order 11 22 33 44 55 11
SETS = [{11, 22, 33}, {11, 44}, {22, 33, 55}, {11}, set(), {44, 55}, {22, 44}, {11, 22, 33, 44, 55}, {99}]
USED = [[0, 1, 2], [0, 3], [1, 2, 4], [0, 5], None, [3, 4], None, [0, 1, 2], None]          # columns; None: the policy is not satisfied


def test_leaf_mask_marks_every_leaf_of_a_repeated_attribute():
    tree = example_tree()
    m = bsw07.leaf_mask(tree, SETS)
    assert m.dtype == np.uint8 and m.tolist() == [[1, 1, 1, 0, 0, 1], [1, 0, 0, 1, 0, 1], [0, 1, 1, 0, 1, 0], [1, 0, 0, 0, 0, 1], [0] * 6, [0, 0, 0, 1, 1, 0],
                                                  [0, 1, 0, 1, 0, 0], [1] * 6, [0] * 6]
    assert (bsw07.leaf_mask(bsw07.share_plan(tree), [sorted(s) for s in SETS]) == m).all()          # a plan, and lists for sets
    assert bsw07.leaf_mask(tree, []).shape == (0, 6)
    assert bsw07.leaf_mask(L("a"), [{"a"}, {"b"}]).tolist() == [[1], [0]]


def test_used_columns_are_compacted_in_leaf_order():
    used = np.array([[0, 1, 0, 1, 1], [0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 7, 0, 255]], dtype=np.uint8)
    index, mask, U = bsw07.used_columns(used)
    assert U == 3 and index.dtype == np.int64 and mask.dtype == np.uint8
    assert index.tolist() == [[1, 3, 4], [0, 0, 0], [0, 0, 0], [2, 4, 0]] and mask.tolist() == [[1, 1, 1], [0, 0, 0], [1, 0, 0], [1, 1, 0]]
    index, mask, U = bsw07.used_columns(np.zeros((2, 4), dtype=np.uint8))
    assert U == 0 and index.shape == (2, 0) and mask.shape == (2, 0)
    assert bsw07.used_columns(np.zeros((0, 4), dtype=np.uint8))[2] == 0


@pytest.fixture(scope="module")
def setup(oracle):
    eng = StandInEngine(oracle)
    eng.pairs = recorded(eng, ("multi_pair",))                               # every list that reaches multi_pair
    inst = Instance(eng, example_tree(), user_attrs=[], n_ct=3)
    picks = [t % 3 for t in range(len(SETS))]
    D, dj, djp, _, _ = user_keys(eng, inst.tree, SETS)
    return eng, inst, picks, bsw07.leaf_mask(inst.tree, SETS), D, dj, djp, ciphertext_arrays(inst, picks)


def test_messages_ok_flags_and_the_lists_that_reach_the_engine(setup):
    eng, inst, picks, held, D, dj, djp, (c_tilde, c, cy, cyp) = setup
    n = len(SETS)
    del eng.pairs[:]
    msgs, ok = bsw07.decrypt_batch_keys(eng, inst.tree, held, D, dj, djp, c_tilde, c, cy, cyp)
    assert msgs.shape == (n, 384) and ok.shape == (n,) and ok.tolist() == [int(u is not None) for u in USED]
    for t in range(n):
        assert msgs[t].tobytes() == (np.asarray(inst.msgs[picks[t]]).tobytes() if USED[t] else bytes(384)), t
    # one multi_pair: a segment per satisfied item, 2 U + 1 pairs with U = 3 and not 2 L + 1 = 13
    (_, (P, Q, off)), = eng.pairs
    P, Q, off = np.asarray(P).reshape(-1, 64), np.asarray(Q).reshape(-1, 128), np.asarray(off)
    good = [t for t in range(n) if USED[t]]
    assert off.tolist() == list(range(0, 7 * len(good) + 1, 7)) and len(P) == len(Q) == 7 * len(good)
    assert not (Q == GARBAGE).all(1).any()                                   # no row of a leaf that is not held went in
    for s, t in enumerate(good):
        cols = USED[t]
        q, p = Q[7 * s:7 * s + 7], P[7 * s:7 * s + 7]
        for i in range(3):
            if i < len(cols):
                assert q[i].tobytes() == dj[t, cols[i]].tobytes() and q[3 + i].tobytes() == djp[t, cols[i]].tobytes(), (t, i)      # stable leaf order
                assert p[i].any() and p[3 + i].any()
            else:
                assert not q[i].any() and not q[3 + i].any() and not p[i].any() and not p[3 + i].any(), (t, i)                      # infinity on both sides
        assert q[6].tobytes() == eng.g2_neg(D[t]).tobytes() and p[6].tobytes() == c[t].tobytes()


def test_one_key_against_many_ciphertexts_and_tensors(setup):
    eng, inst, picks, held, D, dj, djp, (c_tilde, c, cy, cyp) = setup
    # the first user's key against three ciphertexts
    want = np.stack([np.asarray(m) for m in inst.msgs])
    args = (np.tile(held[0], (3, 1)), D[0], np.tile(dj[0], (3, 1, 1)), np.tile(djp[0], (3, 1, 1))) + ciphertext_arrays(inst, [0, 1, 2])
    msgs, ok = bsw07.decrypt_batch_keys(eng, bsw07.share_plan(inst.tree), *args)
    assert ok.tolist() == [1, 1, 1] and msgs.tobytes() == want.tobytes()
    full = (held, D, dj, djp, c_tilde, c, cy, cyp)
    ref = bsw07.decrypt_batch_keys(eng, inst.tree, *full)
    for other in (held != 0, [[bool(v) for v in row] for row in held], held * 0xFF):          # a bool array, nested values, any non-zero byte
        again = bsw07.decrypt_batch_keys(eng, inst.tree, other, *full[1:])
        assert again[0].tobytes() == ref[0].tobytes() and again[1].tobytes() == ref[1].tobytes()
    got = bsw07.decrypt_batch_keys(TensorEngine(eng), inst.tree, *tensors(*full))
    assert same_on_tensors(got[0], ref[0]) and same_on_tensors(got[1], ref[1])
    one = bsw07.decrypt_batch_keys(TensorEngine(eng), inst.tree, *tensors(args[0]), args[1], *tensors(*args[2:]))      # D [128] stays a host value
    assert same_on_tensors(one[0], msgs)


def test_nothing_satisfied_no_items_and_a_single_leaf(setup):
    eng, inst, picks, held, D, dj, djp, (c_tilde, c, cy, cyp) = setup
    bad = [4, 6, 8]
    del eng.pairs[:]
    msgs, ok = bsw07.decrypt_batch_keys(eng, inst.tree, held[bad], D[bad], dj[bad], djp[bad], c_tilde[bad], c[bad], cy[bad], cyp[bad])
    assert not ok.any() and not msgs.any() and msgs.shape == (3, 384) and not eng.pairs                      # no group operation at all
    msgs, ok = bsw07.decrypt_batch_keys(eng, inst.tree, held[:0], D[:0], dj[:0], djp[:0], c_tilde[:0], c[:0], cy[:0], cyp[:0])
    assert msgs.shape == (0, 384) and ok.shape == (0,)
    # the policy that is one leaf: w = 1, so the lists are the ciphertext's own components
    leaf = L(11)
    one = Instance(eng, leaf, user_attrs=[], n_ct=1)
    D1, dj1, djp1, _, _ = user_keys(eng, leaf, [{11}, {22}])
    ct = ciphertext_arrays(one, [0, 0])
    msgs, ok = bsw07.decrypt_batch_keys(eng, leaf, bsw07.leaf_mask(leaf, [{11}, {22}]), D1, dj1, djp1, *ct)
    assert ok.tolist() == [1, 0] and msgs[0].tobytes() == np.asarray(one.msgs[0]).tobytes() and not msgs[1].any()


def test_argument_errors(setup):
    eng, inst, picks, held, D, dj, djp, (c_tilde, c, cy, cyp) = setup
    import torch
    f = lambda **kw: bsw07.decrypt_batch_keys(eng, inst.tree, **{**dict(held=held, d_key=D, dj=dj, dj_prime=djp, c_tilde=c_tilde, c=c, cy=cy, cy_prime=cyp), **kw})
    for kw in (dict(held=held[:, :5]), dict(held=held[:-1]), dict(d_key=D[:2]), dict(d_key=D.reshape(-1)[:-1]), dict(dj=dj[:, :5]), dict(dj_prime=djp[:-1]),
               dict(c_tilde=c_tilde[:-1]), dict(cy=cy[:, :5]), dict(cy_prime=cyp[:, :, :63]), dict(c=c.reshape(-1)[:-1])):
        with pytest.raises(ValueError, match="need held"):
            f(**kw)
    with pytest.raises(ValueError, match="uint8 or bool"):
        f(held=held.astype(np.int32))
    with pytest.raises(ValueError, match="every item needs 6"):
        f(held=[row[:5] for row in held.tolist()])
    with pytest.raises(ValueError, match="all be CUDA tensors or all host"):
        f(cy=torch.from_numpy(cy.copy()))
    with pytest.raises(ValueError, match="all be CUDA tensors or all host"):
        f(d_key=torch.from_numpy(D.copy()))
    with pytest.raises(ValueError, match="names 5 attributes for 6 leaves"):
        nodes, attrs = bsw07.share_plan(inst.tree)
        bsw07.decrypt_batch_keys(eng, (nodes, attrs[:5]), held[:, :5], D, dj[:, :5], djp[:, :5], c_tilde, c, cy[:, :5], cyp[:, :5])
