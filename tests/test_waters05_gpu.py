"""Waters05 IBE batches on the device (run with -m gpu): a seeded instance of 64 identities (waters05_fixture.py) through
waters05.keygen_batch / encrypt_batch / decrypt_batch on the GPU engine, host arrays and CUDA tensors — the keys and ciphertexts
byte-identical to the oracle's evaluation on exponents, every message back from decrypt_batch, and none under another identity's key."""
import numpy as np
import pytest

from waters05_fixture import Instance
from gopairingbasedcryptography_amd import waters05

pytestmark = pytest.mark.gpu
N = 64


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


@pytest.fixture(scope="module")
def inst(oracle):
    return Instance(oracle, ["user-%d@example.com" % i for i in range(N)], tag="gpu")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "cuda"])
def test_keygen_encrypt_decrypt(eng, inst, on_device):
    put = dev if on_device else (lambda a: a)
    host = (lambda a: a.cpu().numpy()) if on_device else (lambda a: a)
    masks = waters05.identity_masks(inst.ids)
    assert masks.shape == (N, 32) and (np.unpackbits(masks, axis=1) == np.array(inst.bits)).all()
    table = waters05.hash_table(eng, put(inst.u_prime), put(inst.ui))
    assert table.table_bytes() == (2 << 20) + 8192
    d1, d2 = waters05.keygen_batch(eng, table, inst.g2_alpha, put(masks), put(inst.rows(inst.r)))
    assert (host(d1) == inst.d1).all() and (host(d2) == inst.d2).all()
    c1, c2, c3 = waters05.encrypt_batch(eng, table, inst.e_alpha, put(inst.messages), put(masks), put(inst.rows(inst.t)))
    assert (host(c1) == inst.c1).all() and (host(c2) == inst.c2).all() and (host(c3) == inst.c3).all()
    if on_device:
        assert all(x.is_cuda for x in (d1, d2, c1, c2, c3))
    assert (host(waters05.decrypt_batch(eng, (d1, d2), c1, c2, c3)) == inst.messages).all()
    # the key of identity 0 against every ciphertext: its own message, and no other
    one = host(waters05.decrypt_batch(eng, (inst.d1[0], inst.d2[0]), c1, c2, c3))
    assert (one[0] == inst.messages[0]).all() and (one[1:] != inst.messages[1:]).any(axis=1).all()
    # every key rolled by one identity: nothing decrypts
    rolled = host(waters05.decrypt_batch(eng, (put(np.roll(inst.d1, 1, axis=0)), put(np.roll(inst.d2, 1, axis=0))), c1, c2, c3))
    assert (rolled != inst.messages).any(axis=1).all()
    # Python integers as the randomness
    assert (host(waters05.keygen_batch(eng, table, inst.g2_alpha, put(masks[:3]), inst.r[:3])[0]) == inst.d1[:3]).all()
    table.close()
