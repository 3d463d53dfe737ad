"""Gentry06 IBE batches (gopairingbasedcryptography_amd/gentry06.py), CPU part: the planner on a stand-in engine — every engine name on
the oracle, H by hashlib — against (a) the on-exponent expectation of gentry06_fixture.py, single generator multiplications that share
nothing with the planner's sequence, and (b) the reference's own sequences of KeyGenerate / Encrypt / Decrypt written out with oracle
calls.  N = 8 identities, k = 1 (gentry06_cpa_ibe) and k = 3 (gentry06_ibe); identity 5 equals alpha, the reference's "ID equals alpha"
error.  The same runs on CPU tensors (standin_engine.TensorEngine) cover the tensor path of the planner without a GPU."""
import numpy as np
import pytest

import gentry06_fixture as gf
from standin_engine import StandInEngine, TensorEngine, same_on_tensors, tensors

N, ALPHA_AT = 8, 5
KS = [1, 3]
_INST = {}


def instance(oracle, k):
    if k not in _INST:
        _INST[k] = gf.Instance(oracle, N, k, alpha_at=ALPHA_AT)
    return _INST[k]


@pytest.fixture(scope="module")
def planner():
    from gopairingbasedcryptography_amd import gentry06
    return gentry06


@pytest.fixture(scope="module")
def eng(oracle):
    return StandInEngine(oracle)


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("k", KS)
def test_keygen_is_the_expectation_and_the_reference_sequence(planner, eng, oracle, k):
    t = instance(oracle, k)
    rids, hids, ok = planner.keygen_batch(eng, t.alpha, t.h, t.ids, t.r)
    assert rids.shape == (N, k, 32) and hids.shape == (N, k, 128) and ok.shape == (N,) and ok.dtype == np.uint8
    assert list(ok) == [int(i != ALPHA_AT) for i in range(N)]
    assert same(rids, t.rids) and same(hids, t.hids)
    assert not rids[ALPHA_AT].any() and not hids[ALPHA_AT].any() and t.reference_keygen(ALPHA_AT) is None     # zero rows, neighbours unaffected
    for i in (0, ALPHA_AT - 1, ALPHA_AT + 1):
        r_ref, h_ref = t.reference_keygen(i)
        assert same(rids[i], r_ref) and same(hids[i], h_ref), i
    # scalar rows in place of integers
    rows = planner.keygen_batch(eng, gf.kbytes([t.alpha]), t.h, gf.kbytes(t.ids), gf.kbytes([x for r in t.r for x in r]))
    assert all(same(a, b) for a, b in zip(rows, (rids, hids, ok)))


@pytest.mark.parametrize("k", KS)
def test_public_pairings(planner, eng, oracle, k):
    t = instance(oracle, k)
    e_gg, e_gh = planner.public_pairings(eng, gf.G1, gf.G2, t.h)
    assert e_gg.shape == (384,) and e_gh.shape == (k, 384) and same(e_gg, t.e) and same(e_gh, t.e_gh)


@pytest.mark.parametrize("k", KS)
def test_encrypt_is_the_expectation_and_the_reference_sequence(planner, eng, oracle, k):
    t = instance(oracle, k)
    ct = planner.encrypt_batch(eng, t.g1_alpha, t.e, t.e_gh, t.messages, t.ids, t.s)
    assert len(ct) == (3 if k == 1 else 4) and [c.shape for c in ct] == [(N, 64)] + [(N, 384)] * (len(ct) - 1)
    for got, want, name in zip(ct, t.ct(), "uvwy"):
        assert same(got, want), name
    assert not ct[0][ALPHA_AT].any()                                          # u = [0] g1: infinity is an ordinary input of H
    for i in (0, ALPHA_AT, N - 1):
        for got, want, name in zip(ct, t.reference_encrypt(i), "uvwy"):
            assert same(got[i], want), (i, name)


@pytest.mark.parametrize("k", KS)
def test_decrypt_per_item_keys_and_one_key(planner, eng, oracle, k):
    t = instance(oracle, k)
    good = t.valid()
    msgs, ok = planner.decrypt_batch(eng, (t.rids[good], t.hids[good]), *t.ct(good))
    assert msgs.shape == (len(good), 384) and ok.shape == (len(good),) and ok.all() and same(msgs, t.messages[good])
    for j, i in enumerate(good[:2]):
        assert same(t.reference_decrypt(t.rids[i], t.hids[i], *(c[0] for c in t.ct([i]))), msgs[j])
    # one key against all ciphertexts: only its own ciphertext passes the check (k = 3) / decrypts (k = 1)
    i = good[2]
    msgs, ok = planner.decrypt_batch(eng, (t.rids[i], t.hids[i]), *t.ct())
    assert same(msgs[i], t.messages[i])
    if k == 3:
        assert list(ok) == [int(j == i) for j in range(N)] and not np.delete(msgs, i, axis=0).any()
        assert t.reference_decrypt(t.rids[i], t.hids[i], *(c[0] for c in t.ct([good[0]]))) is None
    else:
        assert ok.all() and all(not same(msgs[j], t.messages[j]) for j in range(N) if j != i)
    # the key of the identity that equals alpha is all zero: the check refuses its ciphertext
    if k == 3:
        msgs, ok = planner.decrypt_batch(eng, (t.rids, t.hids), *t.ct())
        assert list(ok) == list(t.ok) and not msgs[ALPHA_AT].any() and same(msgs[good], t.messages[good])
    empty = planner.decrypt_batch(eng, (t.rids[i], t.hids[i]), *(c[:0] for c in t.ct()))
    assert empty[0].shape == (0, 384) and empty[1].shape == (0,)


@pytest.mark.parametrize("how", ["y", "w", "u"])
def test_tampering_fails_the_check_and_nothing_else(planner, eng, oracle, how):
    t = instance(oracle, 3)
    good = t.valid()
    ct, spoiled = gf.tamper(t, oracle, how, good)
    msgs, ok = planner.decrypt_batch(eng, (t.rids[good], t.hids[good]), *ct)
    assert list(ok) == [int(j not in spoiled) for j in range(len(good))]
    for j, i in enumerate(good):
        assert (not msgs[j].any()) if j in spoiled else same(msgs[j], t.messages[i]), (how, j)
    assert t.reference_decrypt(t.rids[good[0]], t.hids[good[0]], *(c[0] for c in ct)) is None


@pytest.mark.parametrize("k", KS)
def test_tensor_path_with_cpu_tensors(planner, eng, oracle, k):
    import torch
    t = instance(oracle, k)
    te = TensorEngine(eng)
    good = t.valid()
    h, ids, r, messages, s = tensors(t.h, gf.kbytes(t.ids), gf.kbytes([x for row in t.r for x in row]), t.messages, gf.kbytes(t.s))
    key = planner.keygen_batch(te, t.alpha, h, ids, r)
    assert same_on_tensors(key[0], t.rids) and same_on_tensors(key[1], t.hids) and same_on_tensors(key[2], t.ok)
    e_gg, e_gh = planner.public_pairings(te, gf.G1, gf.G2, h)
    assert same_on_tensors(e_gg, t.e) and same_on_tensors(e_gh, t.e_gh)
    ct = planner.encrypt_batch(te, t.g1_alpha, e_gg, e_gh, messages, ids, s)
    assert all(same_on_tensors(got, want) for got, want in zip(ct, t.ct()))
    sel = torch.tensor(good)
    msgs, ok = planner.decrypt_batch(te, (key[0][sel], key[1][sel]), *(c[sel] for c in ct))
    assert same_on_tensors(msgs, t.messages[good]) and same_on_tensors(ok, np.ones(len(good), dtype=np.uint8))
    msgs, ok = planner.decrypt_batch(te, (t.rids[good[0]], t.hids[good[0]]), *(c[sel] for c in ct))        # a host key beside tensor ciphertexts
    assert isinstance(ok, torch.Tensor) and same_on_tensors(msgs[:1], t.messages[good[:1]]) and (k == 1 or ok.tolist() == [1] + [0] * (len(good) - 1))


def test_malformed_arguments(planner, eng, oracle):
    import torch
    t = instance(oracle, 3)
    z = lambda *s: np.zeros(s, dtype=np.uint8)
    bad = [
        lambda: planner.keygen_batch(eng, t.alpha, t.h[:2], t.ids, t.r),                             # two public points
        lambda: planner.keygen_batch(eng, t.alpha, t.h, t.ids, t.r[:-1]),                            # r does not match the identities
        lambda: planner.keygen_batch(eng, t.alpha, t.h, torch.zeros(N * 32, dtype=torch.uint8), t.r),   # kinds differ
        lambda: planner.public_pairings(eng, gf.G1, z(64), t.h),
        lambda: planner.encrypt_batch(eng, t.g1_alpha, t.e, t.e_gh[:2], t.messages, t.ids, t.s),
        lambda: planner.encrypt_batch(eng, t.g1_alpha, t.e, t.e_gh, t.messages, t.ids, t.s[:-1]),
        lambda: planner.encrypt_batch(eng, t.g1_alpha, t.e, t.e_gh, z(385), t.ids[:1], t.s[:1]),
        lambda: planner.decrypt_batch(eng, (t.rids, t.hids), t.u, t.v, t.w[:-1], t.y),
        lambda: planner.decrypt_batch(eng, (t.rids[:2], t.hids[:2]), t.u, t.v, t.w, t.y),            # neither one key nor one per ciphertext
        lambda: planner.decrypt_batch(eng, (t.rids[0], t.hids[0]), t.u, t.v, t.w),                   # a three-point key without y
        lambda: planner.decrypt_batch(eng, (t.rids, t.hids), torch.from_numpy(t.u.copy()), t.v, t.w, t.y),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d was accepted" % i)
