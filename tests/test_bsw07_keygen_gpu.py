"""BSW07 end to end on the device (run with -m gpu): setup -> keygen_batch for ROWS_G2_TABLE_MIN + 1 users over 5 attributes, whose row
call — 5 bases, a row of users each — runs from the G2 row tables, -> the existing encrypt_batch under the nested example policy of
tests/bsw07_fixture.py -> key_for_leaves -> decrypt_batch_keys.  The keys are byte-equal to the ones tests/bsw07_keys_fixture.py makes
from the discrete logs; every user whose attributes satisfy the policy recovers their message, the others come back with ok = 0; host
arrays and CUDA tensors; the seeded form twice from one seed gives equal keys."""
import numpy as np
import pytest

from bsw07_fixture import example_tree, leaves, sc
from bsw07_keys_fixture import user_keys
from sw05_fixture import kbytes
from gopairingbasedcryptography_amd import bn254 as constants, bsw07, rng

pytestmark = pytest.mark.gpu
ATTRS = [11, 22, 33, 44, 55]
U = min(constants.ROWS_G2_TABLE_MIN, 64) + 1
FIXED = [[], ATTRS, [11], [22, 33], [44], [22, 33, 55], [11, 44], [55]]
SEED = bytes((29 * i + 3) % 256 for i in range(32))


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


@pytest.fixture(scope="module")
def setup(eng):
    rnd = np.random.default_rng(7)
    sets = [set(s) for s in FIXED] + [{a for a in ATTRS if rnd.random() < 0.5} for _ in range(U - len(FIXED))]
    tree = example_tree()
    bsw07.assign_leaf_ids(tree)
    pp, msk = bsw07.setup(eng, sc("alpha"), sc("beta"))
    g1, g2 = eng.generators()
    hk = kbytes([sc("h", a) for a in ATTRS])
    h1 = np.asarray(eng.g1_scalar_mul(np.asarray(g1).reshape(-1), hk)).reshape(len(ATTRS), 64)
    h2 = np.asarray(eng.g2_scalar_mul(np.asarray(g2).reshape(-1), hk)).reshape(len(ATTRS), 128)
    r = kbytes([sc("r-user", u) for u in range(U)]).reshape(U, 32)
    rj = kbytes([sc("rj-user-%d" % u, a) for u in range(U) for a in ATTRS]).reshape(U, len(ATTRS), 32)
    held = np.array([[a in s for a in ATTRS] for s in sets], dtype=np.uint8)
    e = np.asarray(eng.pair_batch(np.asarray(g1).reshape(-1), np.asarray(g2).reshape(-1))).reshape(384)
    msgs = np.asarray(eng.gt_exp(np.tile(e, U), kbytes([sc("keygen-msg", u) for u in range(U)]))).reshape(U, 384)
    s = kbytes([sc("keygen-s", u) for u in range(U)]).reshape(U, 32)
    coeffs = kbytes([sc("keygen-q", i) for i in range(2 * U)]).reshape(U, 2, 32)          # the example tree: two gates of threshold 2
    return tree, sets, pp, msk, {a: h1[i] for i, a in enumerate(ATTRS)}, h2, r, rj, held, msgs, s, coeffs


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_setup_keygen_encrypt_decrypt_round_trip(eng, setup, tensors):
    import torch
    tree, sets, pp, msk, h1, h2, r, rj, held, msgs, s, coeffs = setup
    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if tensors else (lambda a: a)
    back = (lambda t: t.cpu().numpy()) if tensors else np.asarray
    D, dj, djp = bsw07.keygen_batch(eng, msk, put(h2), put(r), put(rj), held=put(held))
    assert tensors == isinstance(D, torch.Tensor) == isinstance(dj, torch.Tensor) and tuple(D.shape) == (U, 128) and tuple(dj.shape) == tuple(djp.shape) == (U, len(ATTRS), 128)
    lheld, ldj, ldjp = bsw07.key_for_leaves(tree, ATTRS, put(held), dj, djp)
    # the keys are the fixture's, made from the discrete logs
    wD, wdj, wdjp, _, _ = user_keys(eng, tree, sets)
    attrs_of_leaves = [l.attribute for l in leaves(tree)]
    hD, hheld, hdj, hdjp = back(D), back(lheld), back(ldj), back(ldjp)
    assert hD.tobytes() == wD.tobytes() and hheld.tolist() == bsw07.leaf_mask(tree, sets).tolist()
    for u in range(U):
        for y, a in enumerate(attrs_of_leaves):
            if a in sets[u]:
                assert hdj[u, y].tobytes() == wdj[u, y].tobytes() and hdjp[u, y].tobytes() == wdjp[u, y].tobytes(), (u, y)
            else:
                assert not hdj[u, y].any() and not hdjp[u, y].any(), (u, y)
    # a ciphertext per user under the policy, with the public key setup made
    ct = bsw07.encrypt_batch(eng, tree, pp["h"], pp["e_alpha"], h1, put(msgs), put(s), put(coeffs))
    out, ok = bsw07.decrypt_batch_keys(eng, tree, lheld, D, ldj, ldjp, *ct)
    out, ok = back(out), back(ok)
    want_ok = [int(bsw07.decrypt_plan(tree, st) is not None) for st in sets]
    assert ok.tolist() == want_ok and 3 <= sum(want_ok) <= U - 3
    for u in range(U):
        assert out[u].tobytes() == (msgs[u].tobytes() if want_ok[u] else bytes(384)), u


def test_seeded_keys_are_reproducible_from_the_seed(eng, setup):
    import torch
    tree, sets, pp, msk, h1, h2, *_ = setup
    a = bsw07.keygen_batch_seeded(eng, msk, h2, U, rng.Randomness(eng, SEED))
    b = bsw07.keygen_batch_seeded(eng, msk, h2, U, rng.Randomness(eng, SEED))
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() and np.asarray(x).any() for x, y in zip(a, b))
    t = bsw07.keygen_batch_seeded(eng, msk, torch.from_numpy(h2).cuda(), U, rng.Randomness(eng, SEED))
    assert all(x.is_cuda and x.cpu().numpy().tobytes() == np.asarray(y).tobytes() for x, y in zip(t, a))
    other = bsw07.keygen_batch_seeded(eng, msk, h2, U, rng.Randomness(eng, bytes(32)))
    assert np.asarray(other[0]).tobytes() != np.asarray(a[0]).tobytes()
