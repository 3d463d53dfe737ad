"""BSW07 Encrypt on the MI355X (run with -m gpu) through gopairingbasedcryptography_amd/bsw07.py: encrypt_batch on the GPU engine, host
arrays and CUDA tensors, returns the fixture's ciphertext bytes for 67 ciphertexts under the example tree and under a 3-of-5 gate over
2-of-3 gates; fold_key + decrypt_batch_arrays then recover every message for a key that holds exactly the threshold, and a key one
attribute short gets no plan."""
import numpy as np
import pytest

from bsw07_fixture import Instance, example_tree
from test_bsw07_encrypt_plan import fixture_arrays, fixture_inputs
import share_cases as sc
from gopairingbasedcryptography_amd import bsw07

pytestmark = pytest.mark.gpu
N = 67


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def nested():
    return bsw07.Threshold(3, *[bsw07.Threshold(2, *[bsw07.Leaf(100 + 3 * g + i) for i in range(3)]) for g in range(5)])


POLICIES = {"example": (example_tree, [22, 33, 55], [22, 33]), "3of5-2of3": (nested, [100, 102, 107, 108, 112, 114], [100, 102, 107, 108, 112])}


@pytest.fixture(scope="module", params=list(POLICIES))
def setup(eng, request):
    make, held, _ = POLICIES[request.param]
    inst = Instance(eng, make(), user_attrs=held, n_ct=N)
    return request.param, inst, fixture_inputs(inst, N)


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_encrypt_then_decrypt(eng, setup, tensors):
    import torch
    name, inst, (s, coeffs, h, h1) = setup
    L = len(bsw07.share_plan(inst.tree)[1])
    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if tensors else (lambda a: a)
    back = (lambda t: t.cpu().numpy()) if tensors else np.asarray
    msgs = np.stack(inst.msgs)
    got = bsw07.encrypt_batch(eng, inst.tree, h, inst.e_alpha, h1, put(msgs), put(sc.rows(s).reshape(N, 32)), put(sc.rows([v for q in coeffs for v in q]).reshape(N, -1, 32)))
    for g, w, shape in zip(got, fixture_arrays(inst), ((N, 384), (N, 64), (N, L, 64), (N, L, 64))):
        assert tuple(g.shape) == shape and (tensors == isinstance(g, torch.Tensor)) and back(g).tobytes() == w.tobytes()
    # a key that satisfies the policy with exactly the threshold recovers every message; one attribute short there is no plan
    plan = bsw07.decrypt_plan(inst.tree, inst.user_attrs)
    assert plan is not None and bsw07.decrypt_plan(inst.tree, set(POLICIES[name][2])) is None
    folded = bsw07.fold_key(eng, plan, inst.dj, inst.dj_prime)
    cols = [i - 1 for i in folded[0]]
    c_tilde, c, cy, cy_prime = got
    pick = (lambda a: a[:, cols].contiguous()) if tensors else (lambda a: np.ascontiguousarray(a[:, cols]))
    out = bsw07.decrypt_batch_arrays(eng, folded, inst.D, c_tilde, c, pick(cy), pick(cy_prime))
    assert back(out).tobytes() == msgs.tobytes()
