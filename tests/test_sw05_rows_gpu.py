"""The SW05 planners from attribute rows on the device (run with -m gpu): the small instances of tests/test_sw05_plan.py on host arrays and
on tensors against the reference's Decrypt loop; the selection alone at 2^14 ciphertexts x 24 attributes against a key of 32, d = 16,
every row against sw05.select_common; both decrypts at the first 2^10 of those ciphertexts, rows form against integer form."""
import numpy as np
import pytest

import bn254_py as o
from sw05_fixture import Instance, at_size_attributes
from test_sw05_plan import KEY, cts_for
from gopairingbasedcryptography_amd import sw05

pytestmark = pytest.mark.gpu
R = o.R


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


@pytest.fixture(scope="module")
def at_size():
    """(key attributes, 2^14 ciphertexts' attributes): every 64th ciphertext shares d - 1 = 15 attributes with the key"""
    return at_size_attributes(1 << 14, 24, 32, 16, every=64)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(eng, inst, ct_attrs, key, put=lambda a: a):
    if inst.n_univ is None:
        return sw05.decrypt_batch(eng, key, inst.d, ct_attrs, put(inst.E), put(inst.e_prime))
    return sw05.decrypt_batch_large(eng, key, inst.d, ct_attrs, put(inst.E), put(inst.e_pp), put(inst.e_prime))


@pytest.mark.parametrize("large", [False, True])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_small_instances_host_and_device(eng, oracle, d, large):
    inst = Instance(eng, d, KEY, cts_for(d), n_univ=5 if large else None, tag="p%d" % d)
    ref = [inst.reference_shaped_decrypt(oracle, t) for t in range(4)]
    assert ref[2] is None
    rows = sw05.attribute_rows(cts_for(d))
    per_item = (np.tile(sw05.attribute_rows(KEY), (4, 1, 1)),) + tuple(np.tile(np.asarray(c), (4, 1, 1)) for c in inst.key[1:])
    for key in (inst.key, (sw05.attribute_rows(KEY),) + tuple(inst.key[1:]), per_item):
        for put, back in ((lambda a: a, np.asarray), (lambda a: to_dev(np.asarray(a)), lambda t: t.cpu().numpy())):
            k = key if isinstance(key[0], list) else tuple(put(c) for c in key)
            out, ok = run(eng, inst, put(rows), k, put)
            assert type(out) is type(put(rows)) and type(ok) is type(out)
            out, ok = back(out), back(ok)
            assert ok.tolist() == [1, 1, 0, 1] and not out[2].any()
            for t in (0, 1, 3):
                assert (out[t] == np.asarray(inst.msgs)[t]).all() and (out[t] == ref[t]).all(), t


def test_selection_at_2_14(eng, at_size):
    """every row of the device's selection against sw05.select_common; ok = 0 for exactly the 256 ciphertexts below the threshold"""
    key_attrs, cts = at_size
    n, a, m, d = 1 << 14, 24, 32, 16
    kp, cp, want_ok = sw05.select_common(key_attrs, cts, d)
    below = np.arange(n) % 64 == 63
    assert (want_ok == (~below).astype(np.uint8)).all()
    S, L = sw05.attribute_rows(key_attrs), sw05.attribute_rows(cts)
    want_common = L.reshape(n * a, 32)[(np.arange(n)[:, None] * a + cp).reshape(-1)].reshape(n, d, 32) * want_ok[:, None, None]
    for put, back in ((lambda x: x, np.asarray), (to_dev, lambda t: t.cpu().numpy())):
        sp, lp, common, ok = [back(r) for r in eng.fr_find_common(put(S.reshape(-1)), put(L.reshape(-1)), m, a, d)]
        assert (ok == want_ok).all() and int((ok == 0).sum()) == 256
        assert (sp == kp).all() and (lp == cp).all() and common.tobytes() == want_common.tobytes()
        assert not sp[below].any() and not lp[below].any() and not common[below].any()


@pytest.mark.parametrize("large", [False, True])
def test_decrypts_at_2_10_rows_form_is_integer_form(eng, at_size, large):
    import torch
    key_attrs, cts = at_size
    n, a, d = 1 << 10, 24, 16
    cts = cts[:n]
    dev = torch.device("cuda", 0)
    inst = Instance(eng, d, key_attrs, cts, n_univ=a if large else None, dev=dev, tag="rows")
    try:
        want, want_ok = run(eng, inst, cts, inst.key)
        below = np.arange(n) % 64 == 63
        rows = to_dev(sw05.attribute_rows(cts))
        for key in (inst.key, (to_dev(sw05.attribute_rows(key_attrs)),) + tuple(to_dev(c) for c in inst.key[1:])):
            out, ok = run(eng, inst, rows, key)
            assert out.is_cuda and ok.is_cuda and ok.dtype == torch.uint8
            assert (ok.cpu().numpy() == (~below).astype(np.uint8)).all() and torch.equal(ok, want_ok)
            assert torch.equal(out, want)                                                            # byte for byte
            zero = (out == 0).all(dim=1).cpu().numpy()
            assert np.nonzero(zero)[0].tolist() == np.nonzero(below)[0].tolist() and int(zero.sum()) == 16
        assert torch.equal(want[torch.from_numpy(np.nonzero(~below)[0]).to(dev)], inst.msgs.reshape(n, 384)[torch.from_numpy(np.nonzero(~below)[0]).to(dev)])
    finally:
        eng.release_workspaces()
