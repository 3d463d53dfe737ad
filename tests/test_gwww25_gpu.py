"""GWWW25 batched IBE on the MI355X (run with -m gpu): gopairingbasedcryptography_amd/gwww25.py over the engine itself, B = 16 with batches of
16, 7 and 1 identities.  Every digest, key and ciphertext component is held against the transcription of gwww25_bibe.go in
tests/gwww25_reference.py (the C oracle and Python integers) — never against the code under test; the round trip decrypt(encrypt(M)) == M
runs on host arrays and on CUDA tensors, with the Encrypt tables and without; a batch list with a repeated identity gives ok = 0 and zero
messages on both copies while its neighbours decrypt to what the reference gives for that list."""
import numpy as np
import pytest

from gwww25_reference import G1, G2, Ref, R, row, sc
from sw05_fixture import kbytes

pytestmark = pytest.mark.gpu
B = 16
COUNTS = [16, 7, 1]
SAMPLE = [0, 9, 15, 16, 22, 23]                                       # the items the per-item transcription is run on


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def world(eng, oracle):
    """keys, tables, ciphertexts and secret keys of the three batches, made once by the planner on host arrays"""
    from gopairingbasedcryptography_amd import gwww25
    ref = Ref(oracle, B)
    n = sum(COUNTS)
    w = dict(ref=ref, n=n, ids=[sc("gpu-id", i) for i in range(n)], of_item=np.repeat(np.arange(len(COUNTS)), COUNTS),
             tg=[sc("gpu-tg", j) for j in range(len(COUNTS))], s=[sc("gpu-s", i) for i in range(n)],
             r=[sc("gpu-r", j) for j in range(len(COUNTS))], y=[sc("gpu-y", j) for j in range(len(COUNTS))])
    w["mpk"] = gwww25.keygen(eng, B, ref.tau, ref.w, ref.v, ref.h, ref.alpha)
    w["table"] = gwww25.srs_table(eng, w["mpk"])
    w["tables"] = gwww25.encrypt_tables(eng, w["mpk"])
    e = np.asarray(eng.pair_batch(G1, G2)).reshape(384)
    w["messages"] = np.asarray(eng.gt_exp(np.tile(e, n), kbytes([sc("gpu-msg", i) for i in range(n)]))).reshape(n, 384)
    w["tg_items"] = kbytes([w["tg"][j] for j in w["of_item"]])
    w["D"] = gwww25.digests(eng, w["table"], kbytes(w["ids"]), COUNTS)
    w["sk"] = gwww25.compute_key_batch(eng, (ref.w, ref.v, ref.h, ref.alpha), w["D"], w["tg"], w["r"], w["y"])
    w["ct"] = gwww25.encrypt_batch(eng, w["mpk"], w["messages"], kbytes(w["ids"]), w["tg_items"], kbytes(w["s"]))
    yield w
    for t in (w["table"],) + tuple(w["tables"]):
        t.close()


def test_keys_digests_and_ciphertexts_are_the_reference(eng, world):
    from gopairingbasedcryptography_amd import gwww25
    ref, mpk = world["ref"], world["mpk"]
    assert mpk["G2ExpTauPowers"].tobytes() == np.stack(ref.powers).tobytes() and mpk["GTExpAlpha"].tobytes() == ref.gt_alpha.tobytes()
    assert all(mpk[k].tobytes() == v.tobytes() for k, v in (("G1ExpTau", ref.g1_tau), ("G1ExpW", ref.g1_w), ("G1ExpWTau", ref.g1_wtau), ("G1ExpV", ref.g1_v), ("G1ExpH", ref.g1_h)))
    ids, K = world["ids"], kbytes(world["ids"])
    D = world["D"]
    a = 0
    for j, c in enumerate(COUNTS):
        assert D[j].tobytes() == ref.digest(ids[a:a + c]).tobytes(), j
        a += c
    assert gwww25.digests(eng, world["table"], to_dev(K), COUNTS).cpu().numpy().tobytes() == D.tobytes()
    msk = (ref.w, ref.v, ref.h, ref.alpha)
    y, u1, u2 = world["sk"]
    for j in range(len(COUNTS)):
        _, ru1, ru2 = ref.compute_key(D[j], world["tg"][j], world["r"][j], world["y"][j])
        assert u1[j].tobytes() == ru1.tobytes() and u2[j].tobytes() == ru2.tobytes(), j
    dy, du1, du2 = gwww25.compute_key_batch(eng, msk, to_dev(D), to_dev(kbytes(world["tg"])), to_dev(kbytes(world["r"])), to_dev(kbytes(world["y"])))
    assert du1.cpu().numpy().tobytes() == u1.tobytes() and du2.cpu().numpy().tobytes() == u2.tobytes()
    ct = world["ct"]
    for i in SAMPLE:
        want = ref.encrypt(world["messages"][i], ids[i], world["tg"][world["of_item"][i]], world["s"][i])
        assert all(ct[t][i].tobytes() == want[t].tobytes() for t in range(4)), i
    fast = gwww25.encrypt_batch(eng, mpk, world["messages"], K, world["tg_items"], kbytes(world["s"]), tables=world["tables"])
    dev = gwww25.encrypt_batch(eng, mpk, to_dev(world["messages"]), to_dev(K), to_dev(world["tg_items"]), to_dev(kbytes(world["s"])), tables=world["tables"])
    assert all(f.tobytes() == c.tobytes() and d.cpu().numpy().tobytes() == c.tobytes() for f, d, c in zip(fast, dev, ct))


def test_round_trip_and_rejected_rows(eng, world):
    from gopairingbasedcryptography_amd import gwww25
    ref, ids, K, table, sk, ct = world["ref"], world["ids"], kbytes(world["ids"]), world["table"], world["sk"], world["ct"]
    m, ok = gwww25.decrypt_batches(eng, table, K, COUNTS, sk, ct)
    assert ok.tolist() == [1] * world["n"] and m.tobytes() == world["messages"].tobytes()
    dm, dok = gwww25.decrypt_batches(eng, table, to_dev(K), COUNTS, tuple(to_dev(x) for x in sk), tuple(to_dev(x) for x in ct))
    assert dm.is_cuda and dok.is_cuda and dm.cpu().numpy().tobytes() == m.tobytes() and dok.cpu().numpy().tolist() == ok.tolist()
    i = 20                                                             # an item of the batch of 7, through the reference's Decrypt
    key = (world["y"][1], sk[1][1], sk[2][1])
    assert m[i].tobytes() == ref.decrypt(key, ids[16:23], ids[i], tuple(c[i] for c in ct)).tobytes()
    # the batch of 7 with its third identity repeated in fifth place: both copies are refused, the others give what the reference gives
    dup = list(ids)
    dup[16 + 4] = dup[16 + 2]
    m2, ok2 = gwww25.decrypt_batches(eng, table, to_dev(kbytes(dup)), COUNTS, tuple(to_dev(x) for x in sk), tuple(to_dev(x) for x in ct))
    m2, ok2 = m2.cpu().numpy(), ok2.cpu().numpy()
    want_ok = np.ones(world["n"], dtype=np.uint8)
    want_ok[[18, 20]] = 0
    assert ok2.tolist() == want_ok.tolist() and not m2[18].any() and not m2[20].any()
    assert m2[:16].tobytes() == m[:16].tobytes() and m2[23].tobytes() == m[23].tobytes()
    assert m2[17].tobytes() == ref.decrypt(key, dup[16:23], dup[17], tuple(c[17] for c in ct)).tobytes() and m2[17].tobytes() != m[17].tobytes()
    with pytest.raises(ValueError, match="identity not found"):
        ref.decrypt(key, dup[16:23], dup[18], tuple(c[18] for c in ct))
    assert R > max(ids)
