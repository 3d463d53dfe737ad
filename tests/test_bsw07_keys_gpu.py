"""BSW07 decryption with a key per item on the MI355X (run with -m gpu) through bsw07.decrypt_batch_keys: 24 users with attribute sets
of their own under the example tree and under a 3-of-5 gate over 2-of-3 gates, keys and ciphertexts from the known secrets of
tests/bsw07_fixture.py, host arrays and CUDA tensors.  The ok flags are those of bsw07.decrypt_plan; every ok = 1 message is the
original message and, byte for byte, what the existing one-key route (decrypt_plan + fold_key + decrypt_batch) gives for that user."""
import numpy as np
import pytest

from bsw07_fixture import Instance, example_tree
from bsw07_keys_fixture import ciphertext_arrays, user_keys
from test_bsw07_encrypt_gpu import nested
from gopairingbasedcryptography_amd import bsw07

pytestmark = pytest.mark.gpu
N, N_CT = 24, 4


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def attribute_sets(universe, density, seed, fixed):
    rng = np.random.default_rng(seed)
    sets = [set(s) for s in fixed]
    while len(sets) < N:
        sets.append({a for a in universe if rng.random() < density})
    return sets


POLICIES = {
    "example": (example_tree, lambda: attribute_sets([11, 22, 33, 44, 55], 0.5, 7, [[], [11, 22, 33, 44, 55], [11], [22, 33], [44], [22, 33, 55], [99]])),
    "3of5-2of3": (nested, lambda: attribute_sets(range(100, 115), 0.55, 8, [[], range(100, 115), [100, 102, 107, 108, 112, 114], [100, 102, 107, 108, 112], [101, 102, 104, 105, 113, 114]])),
}


@pytest.fixture(scope="module", params=list(POLICIES))
def setup(eng, request):
    make, sets = POLICIES[request.param]
    sets = sets()
    inst = Instance(eng, make(), user_attrs=[], n_ct=N_CT)
    picks = [t % N_CT for t in range(N)]
    keys = user_keys(eng, inst.tree, sets)
    plans = [bsw07.decrypt_plan(inst.tree, s) for s in sets]
    one_key = []                                                             # the existing route, a user at a time
    for t, plan in enumerate(plans):
        if plan is None:
            one_key.append(None)
            continue
        folded = bsw07.fold_key(eng, plan, keys[3][t], keys[4][t])
        one_key.append(np.asarray(bsw07.decrypt_batch(eng, folded, keys[0][t], [inst.cts[picks[t]]], Instance.neg_g1)).reshape(384))
    return inst, sets, picks, keys, plans, one_key


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_decrypt_batch_keys(eng, setup, tensors):
    import torch
    inst, sets, picks, (D, dj, djp, _, _), plans, one_key = setup
    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if tensors else (lambda a: a)
    back = (lambda t: t.cpu().numpy()) if tensors else np.asarray
    want_ok = [int(p is not None) for p in plans]
    assert 4 <= sum(want_ok) <= N - 4                                         # both kinds of user, several of each
    held = bsw07.leaf_mask(inst.tree, sets)
    ct = ciphertext_arrays(inst, picks)
    msgs, ok = bsw07.decrypt_batch_keys(eng, inst.tree, put(held), put(D), put(dj), put(djp), *[put(a) for a in ct])
    assert tensors == isinstance(msgs, torch.Tensor) == isinstance(ok, torch.Tensor) and tuple(msgs.shape) == (N, 384) and tuple(ok.shape) == (N,)
    msgs, ok = back(msgs), back(ok)
    assert ok.tolist() == want_ok
    for t in range(N):
        if want_ok[t]:
            assert msgs[t].tobytes() == np.asarray(inst.msgs[picks[t]]).tobytes(), t
            assert msgs[t].tobytes() == one_key[t].tobytes(), t
        else:
            assert not msgs[t].any(), t


def test_one_key_for_all_items(eng, setup):
    """d_key as one [128] value: a user's key against all four ciphertexts"""
    inst, sets, picks, (D, dj, djp, _, _), plans, one_key = setup
    u = next(t for t, p in enumerate(plans) if p is not None and t > 1)
    held = bsw07.leaf_mask(inst.tree, [sets[u]] * N_CT)
    msgs, ok = bsw07.decrypt_batch_keys(eng, bsw07.share_plan(inst.tree), held, D[u], np.tile(dj[u], (N_CT, 1, 1)), np.tile(djp[u], (N_CT, 1, 1)),
                                        *ciphertext_arrays(inst, range(N_CT)))
    assert ok.tolist() == [1] * N_CT and msgs.tobytes() == np.stack([np.asarray(m) for m in inst.msgs]).tobytes()
