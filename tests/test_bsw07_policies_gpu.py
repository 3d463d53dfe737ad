"""BSW07 with a policy per ciphertext on the MI355X (run with -m gpu) through bsw07.encrypt_batch_policies, encrypt_batch_policies_seeded
and decrypt_batch_policies: the 12 items over 3 policies of tests/bsw07_policies_fixture.py (the example tree, 2-of-3, a single leaf; 8
attribute sets that satisfy their policy and 4 that do not), host arrays and CUDA tensors, the variable-base route and the table route.
The ciphertexts equal per-policy encrypt_batch byte for byte with all-zero padding, the seeded form is reproducible from its seed, and
decryption recovers the 8 messages and zeroes the 4."""
import numpy as np
import pytest

from bsw07_policies_fixture import N, POLICY_OF, WANT_OK, Setup, same_as_per_policy
from gopairingbasedcryptography_amd import bsw07, rng

pytestmark = pytest.mark.gpu
SEED = bytes((11 * i + 5) % 256 for i in range(32))


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


@pytest.fixture(scope="module")
def setup(eng):
    st = Setup(eng)
    st.per = [st.per_policy(eng, t) for t in range(3)]
    return st


def forms(tensors):
    import torch
    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if tensors else (lambda a: a)
    ids = (lambda a: put(np.ascontiguousarray(a, dtype=np.uint32).view(np.uint8)).view(torch.int32)) if tensors else (lambda a: a)
    back = (lambda t: t.cpu().numpy()) if tensors else np.asarray
    return put, ids, back


@pytest.mark.parametrize("tables", [False, True], ids=["var-base", "tables"])
@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_encrypt_then_decrypt(eng, setup, tensors, tables):
    import torch
    st = setup
    put, ids, back = forms(tensors)
    got = bsw07.encrypt_batch_policies(eng, st.plan, ids(st.policy_of), st.h, st.e_alpha, st.h1, put(st.msgs), put(st.s), put(st.coeffs), tables=tables)
    assert all(tensors == isinstance(g, torch.Tensor) for g in got)
    assert same_as_per_policy(st, got, st.per, back)
    msgs, ok = bsw07.decrypt_batch_policies(eng, st.plan, ids(st.policy_of), put(st.held), put(st.D), put(st.dj), put(st.djp), *got)
    assert tensors == isinstance(msgs, torch.Tensor) == isinstance(ok, torch.Tensor) and tuple(msgs.shape) == (N, 384) and tuple(ok.shape) == (N,)
    msgs, ok = back(msgs), back(ok)
    assert ok.tolist() == WANT_OK and sum(WANT_OK) == 8
    for i in range(N):
        assert msgs[i].tobytes() == (st.msgs[i].tobytes() if WANT_OK[i] else bytes(384)), i


def test_per_policy_tables_route_agrees(eng, setup):
    """per-policy encrypt_batch with tables=True: the same reference through the other route"""
    for t in range(3):
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(setup.per_policy(eng, t, tables=True), setup.per[t])), t


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_seeded_is_reproducible_from_its_seed(eng, setup, tensors):
    st = setup
    put, ids, back = forms(tensors)
    r = rng.Randomness(eng, SEED)
    first = bsw07.encrypt_batch_policies_seeded(eng, st.plan, ids(st.policy_of), st.h, st.e_alpha, st.h1, put(st.msgs), r)
    assert r.next_stream == 2                                                          # s, then coeffs [n, Cmax]
    again = bsw07.encrypt_batch_policies_seeded(eng, st.trees, POLICY_OF, st.h, st.e_alpha, st.h1, put(st.msgs), rng.Randomness(eng, SEED), tables=True)
    assert all(back(a).tobytes() == back(b).tobytes() for a, b in zip(first, again))
    later = bsw07.encrypt_batch_policies_seeded(eng, st.plan, ids(st.policy_of), st.h, st.e_alpha, st.h1, put(st.msgs), r)
    assert r.next_stream == 4 and all(back(a).tobytes() != back(b).tobytes() for a, b in zip(first, later))
    # the drawn scalars are those of fr_random on the documented streams, and the ciphertexts decrypt
    s, q = eng.fr_random(SEED, N, stream=0), eng.fr_random(SEED, N * st.Cmax, stream=1)
    want = bsw07.encrypt_batch_policies(eng, st.plan, st.policy_of, st.h, st.e_alpha, st.h1, st.msgs, np.asarray(s).reshape(N, 32), np.asarray(q).reshape(N, st.Cmax, 32))
    assert all(back(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(first, want))
    msgs, ok = bsw07.decrypt_batch_policies(eng, st.plan, ids(st.policy_of), put(st.held), put(st.D), put(st.dj), put(st.djp), *first)
    assert back(ok).tolist() == WANT_OK and all(back(msgs)[i].tobytes() == st.msgs[i].tobytes() for i in range(N) if WANT_OK[i])
