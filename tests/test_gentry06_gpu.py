"""Gentry06 IBE batches on the device (run with -m gpu): the seeded instance of gentry06_fixture.py at N = 16 through gentry06.py with
the real engine, k = 1 (gentry06_cpa_ibe) and k = 3 (gentry06_ibe), host arrays and CUDA tensors.  Keys and ciphertexts are byte for byte
the on-exponent expectation (single generator multiplications by the oracle, beta by hashlib); every message of a valid identity comes
back with ok = 1; each of the three tamperings gives ok = 0 and an all-zero row and spoils nothing else; on the CUDA path every output
is a CUDA tensor."""
import numpy as np
import pytest

import gentry06_fixture as gf

pytestmark = pytest.mark.gpu
N, ALPHA_AT = 16, 11
KS = [1, 3]
KINDS = ["host", "cuda"]
_INST = {}


def instance(oracle, k):
    if k not in _INST:
        _INST[k] = gf.Instance(oracle, N, k, tag="gpu-", alpha_at=ALPHA_AT)
    return _INST[k]


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


@pytest.fixture(scope="module")
def planner():
    from gopairingbasedcryptography_amd import gentry06
    return gentry06


def put(kind, *arrays):
    if kind == "host":
        return [np.ascontiguousarray(a) for a in arrays]
    import torch
    return [torch.from_numpy(np.array(a, copy=True)).cuda() for a in arrays]


def host(kind, x):
    if kind == "host":
        assert isinstance(x, np.ndarray)
        return x
    assert x.is_cuda
    return x.cpu().numpy()


def same(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", KS)
def test_keygen_encrypt_decrypt(eng, planner, oracle, k, kind):
    t = instance(oracle, k)
    h, ids, r, messages, s = put(kind, t.h, gf.kbytes(t.ids), gf.kbytes([x for row in t.r for x in row]), t.messages, gf.kbytes(t.s))
    rids, hids, ok = planner.keygen_batch(eng, t.alpha, h, ids, r)
    assert same(host(kind, rids), t.rids) and same(host(kind, hids), t.hids) and same(host(kind, ok), t.ok)
    assert not host(kind, hids)[ALPHA_AT].any() and not host(kind, rids)[ALPHA_AT].any()
    e_gg, e_gh = planner.public_pairings(eng, gf.G1, gf.G2, h)
    assert same(host(kind, e_gg), t.e) and same(host(kind, e_gh), t.e_gh)
    ct = planner.encrypt_batch(eng, t.g1_alpha, e_gg, e_gh, messages, ids, s)
    assert len(ct) == (3 if k == 1 else 4)
    for got, want, name in zip(ct, t.ct(), "uvwy"):
        assert same(host(kind, got), want), name
    good = t.valid()
    sel = good if kind == "host" else put(kind, np.array(good))[0]
    msgs, ok = planner.decrypt_batch(eng, (rids[sel], hids[sel]), *(c[sel] for c in ct))                   # one key per ciphertext
    assert same(host(kind, msgs), t.messages[good]) and host(kind, ok).tolist() == [1] * len(good)
    i = good[3]
    msgs, ok = planner.decrypt_batch(eng, (t.rids[i], t.hids[i]), *ct)                                       # one (host) key for all
    msgs, ok = host(kind, msgs), host(kind, ok)
    assert same(msgs[i], t.messages[i])
    if k == 3:
        assert ok.tolist() == [int(j == i) for j in range(N)] and not np.delete(msgs, i, axis=0).any()
    else:
        assert ok.all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("how", ["y", "w", "u"])
def test_tampering(eng, planner, oracle, how, kind):
    t = instance(oracle, 3)
    good = t.valid()
    ct, spoiled = gf.tamper(t, oracle, how, good)
    rids, hids, *ct = put(kind, t.rids[good], t.hids[good], *ct)
    msgs, ok = planner.decrypt_batch(eng, (rids, hids), *ct)
    msgs, ok = host(kind, msgs), host(kind, ok)
    assert ok.tolist() == [int(j not in spoiled) for j in range(len(good))]
    for j, i in enumerate(good):
        assert (not msgs[j].any()) if j in spoiled else same(msgs[j], t.messages[i]), (how, j)
