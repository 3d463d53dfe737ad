"""The Boneh-Franklin planner (bf01.py) on the oracle stand-in engine (tests/standin_mask.py): KeyGenerate, Encrypt and Decrypt are, byte
for byte, the reference's formulas computed by the oracle in the reference's order — pair, then gt_exp, then bytes
(tests/bf01_fixture.py) — although the planner reaches gid through a G1 scalar multiplication; the round trip; r = 0; a wrong key; the
seeded form; host arrays against tensors; and the engine calls of a one-key Decrypt.  The same instance runs on the GPU engine in
test_bf01_gpu.py."""
import numpy as np
import pytest

import bn254_py as o
import chacha_cases as cc
import mask_cases as mc
from bf01_fixture import DST, Instance, flat_messages
from standin_engine import TensorEngine, recorded, same_on_tensors, tensors
from standin_mask import MaskStandIn
from sw05_fixture import kbytes
from gopairingbasedcryptography_amd import bf01, hash_to, rng

SEED = bytes((11 * i + 5) % 256 for i in range(32))
N = 5


@pytest.fixture(scope="module")
def eng(oracle):
    return MaskStandIn(oracle)


@pytest.fixture(scope="module")
def inst(oracle):
    return Instance(oracle, N)


def same(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_fixture_has_the_five_lengths_and_the_reference_tag(inst):
    assert [len(m) for m in inst.msgs] == [0, 5, 32, 100, 400] and inst.c2_len.tolist() == [0, 5, 32, 100, 384]
    assert DST == hash_to.DST_STRING_G2 == bf01.DST_STRING_G2 and b"ibe Encryption" not in DST
    assert "UNUSED" in bf01.__doc__ and "ibe Encryption" in bf01.__doc__ and "bf01_ibe.go" in bf01.__doc__


def test_keygen_is_the_reference(eng, inst):
    assert same(bf01.identities_to_g2(eng, inst.ids), inst.qids)
    data, off = flat_messages(inst.id_bytes)
    assert same(bf01.identities_to_g2(eng, data, off), inst.qids)                          # a flat buffer plus offsets
    assert same(bf01.identities_to_g2(eng, inst.id_bytes), inst.qids)                      # bytes
    assert same(bf01.public_params(eng, inst.x), inst.g1x) and same(bf01.public_params(eng, kbytes([inst.x])), inst.g1x)
    assert same(bf01.keygen_batch(eng, inst.x, ids=inst.ids), inst.sk)
    assert same(bf01.keygen_batch(eng, kbytes([inst.x]), qids=inst.qids), inst.sk)
    assert bf01.keygen_batch(eng, inst.x, ids=[]).shape == (0, 128)
    with pytest.raises(ValueError):
        bf01.keygen_batch(eng, inst.x)
    with pytest.raises(ValueError):
        bf01.keygen_batch(eng, inst.x, ids=inst.ids, qids=inst.qids)


def test_encrypt_is_the_reference_in_its_order_of_operations(eng, inst):
    """pair, gt_exp, bytes on the oracle's side; g1_scalar_mul, pair_batch, gt_xor_mask on the planner's"""
    c1, (c2, off), c2_len = bf01.encrypt_batch(eng, inst.g1x, inst.msgs, inst.r, ids=inst.ids)
    assert same(c1, inst.c1) and same(c2, inst.c2_data) and same(off, inst.off) and same(c2_len, inst.c2_len)
    c1, c2, c2_len = bf01.encrypt_batch(eng, inst.g1x, inst.data, kbytes(inst.r), qids=inst.qids, msg_off=inst.off)
    assert same(c1, inst.c1) and same(c2, inst.c2_data) and same(c2_len, inst.c2_len)
    with pytest.raises(ValueError):
        bf01.encrypt_batch(eng, inst.g1x, inst.msgs, inst.r[:-1], ids=inst.ids)
    c1, (c2, off), c2_len = bf01.encrypt_batch(eng, inst.g1x, [], [], ids=[])
    assert c1.shape == (0, 64) and c2.size == 0 and c2_len.shape == (0,)


def test_rows_of_one_width(eng, inst, oracle):
    """the row form: five 32-byte messages as [5, 32]"""
    rows = np.stack([np.frombuffer(mc.message("bf01-rows", i, 32), dtype=np.uint8) for i in range(N)])
    c1, c2, c2_len = bf01.encrypt_batch(eng, inst.g1x, rows, inst.r, qids=inst.qids)
    want = np.stack([np.frombuffer(mc.xor_cut(r.tobytes(), k)[0], dtype=np.uint8) for r, k in zip(rows, inst.masks)])
    assert same(c1, inst.c1) and same(c2, want) and c2_len.tolist() == [32] * N
    m, lens = bf01.decrypt_batch(eng, inst.sk, c1, c2)
    assert same(m, rows) and lens.tolist() == [32] * N


def test_decrypt_is_the_reference_and_the_round_trip_recovers_the_message(eng, inst):
    m, lens = bf01.decrypt_batch(eng, inst.sk, inst.c1, inst.c2_data, inst.off)           # a key per ciphertext
    assert same(m, inst.dec_data) and same(lens, inst.c2_len)
    assert inst.dec == inst.recovered() and inst.dec[4][:384] == inst.msgs[4][:384] and inst.dec[4][384:] == bytes(16)
    ct = bf01.encrypt_batch(eng, inst.g1x, inst.msgs, inst.r, ids=inst.ids)
    m, lens = bf01.decrypt_batch(eng, inst.sk, ct[0], ct[1])                               # C2 as encrypt_batch returned it
    assert same(m, inst.dec_data) and same(lens, inst.c2_len)


def test_one_key_for_all_uses_the_fixed_q_pairing_and_nothing_else(oracle, inst):
    """n ciphertexts to ONE identity under its one key: multi_pair_fixed_q + gt_xor_mask, byte-equal to the per-item route"""
    eng = MaskStandIn(oracle)
    q0 = np.tile(inst.qids[0], (N, 1))
    c1, c2, c2_len = bf01.encrypt_batch(eng, inst.g1x, inst.data, inst.r, qids=q0, msg_off=inst.off)
    calls = recorded(eng, [name for name in dir(eng) if not name.startswith("_") and callable(getattr(eng, name))])
    m, lens = bf01.decrypt_batch(eng, inst.sk[0], c1, c2, inst.off)
    assert [name for name, _ in calls] == ["multi_pair_fixed_q", "gt_xor_mask"]
    assert np.asarray(calls[0][1][1]).size == 128                                          # m = 1: the one shared G2 point
    want = [m_[:384] + bytes(max(0, len(m_) - 384)) for m_ in inst.msgs]
    assert m.tobytes() == b"".join(want) and same(lens, inst.c2_len)
    m2, lens2 = bf01.decrypt_batch(eng, inst.sk[:1], c1, c2, inst.off)                     # [1, 128] is the same one key
    m3, lens3 = bf01.decrypt_batch(eng, np.tile(inst.sk[0], (N, 1)), c1, c2, inst.off)     # ... and so is a copy per ciphertext
    assert same(m2, m) and same(m3, m) and same(lens2, lens) and same(lens3, lens)
    assert [name for name, _ in calls] == ["multi_pair_fixed_q", "gt_xor_mask"] * 2 + ["pair_batch", "gt_xor_mask"]


def test_r_zero_gives_infinity_and_the_mask_of_one(eng, inst):
    r = list(inst.r)
    r[4] = 0
    c1, (c2, off), c2_len = bf01.encrypt_batch(eng, inst.g1x, inst.msgs, r, ids=inst.ids)
    one = o.gt_to_canonical_bytes(o.F12_ONE)
    assert not c1[4].any() and c1[3].any()
    a, b = int(off[4]), int(off[5])
    msg = inst.msgs[4]
    assert c2[a:b].tobytes() == mc.xor_cut(msg, one)[0] == msg[:383] + bytes([msg[383] ^ 1]) + bytes(16)
    assert same(c2[:a], inst.c2_data[:a]) and int(c2_len[4]) == 384


def test_wrong_key_does_not_recover(eng, inst):
    wrong = np.roll(inst.sk, 1, axis=0)
    m, lens = bf01.decrypt_batch(eng, wrong, inst.c1, inst.c2_data, inst.off)
    assert same(lens, inst.c2_len)                                                          # no check, no ok: just other bytes
    for i in range(1, N):
        a, b = int(inst.off[i]), int(inst.off[i + 1])
        assert m[a:b].tobytes()[:384] != inst.msgs[i][:384], i


def test_seeded_is_encrypt_batch_on_the_drawn_scalars(oracle, inst):
    eng = MaskStandIn(oracle)
    rnd = rng.Randomness(eng, SEED)
    got = bf01.encrypt_batch_seeded(eng, inst.g1x, inst.msgs, rnd, ids=inst.ids)
    assert eng.draws == [(N, 0, 0)] and rnd.next_stream == 1                               # ONE draw: r [n]
    drawn = cc.scalars(SEED, 0, 0, N)
    want = bf01.encrypt_batch(eng, inst.g1x, inst.msgs, drawn, ids=inst.ids)
    assert same(got[0], want[0]) and same(got[1][0], want[1][0]) and same(got[1][1], want[1][1]) and same(got[2], want[2])
    again = bf01.encrypt_batch_seeded(eng, inst.g1x, inst.data, rnd, qids=inst.qids, msg_off=inst.off)
    assert eng.draws[1:] == [(N, 1, 0)] and rnd.next_stream == 2 and not same(again[0], got[0])
    none = bf01.encrypt_batch_seeded(eng, inst.g1x, [], rnd, ids=[])
    assert none[0].shape == (0, 64) and rnd.next_stream == 2 and len(eng.draws) == 2       # n == 0 takes no stream
    assert "ONE draw" in bf01.encrypt_batch_seeded.__doc__


def test_host_arrays_and_tensors_agree(oracle, inst):
    import torch
    eng = TensorEngine(MaskStandIn(oracle))
    data, qids, sk, g1x, r = tensors(inst.data, inst.qids, inst.sk, inst.g1x, kbytes(inst.r).reshape(N, 32))
    off = torch.from_numpy(inst.off.astype(np.int64))
    assert same_on_tensors(bf01.keygen_batch(eng, inst.x, qids=qids), inst.sk)
    c1, c2, c2_len = bf01.encrypt_batch(eng, g1x, data, r, qids=qids, msg_off=off)
    assert same_on_tensors(c1, inst.c1) and same_on_tensors(c2, inst.c2_data)
    assert isinstance(c2_len, torch.Tensor) and c2_len.numpy().astype(np.uint32).tolist() == inst.c2_len.tolist()
    c1b, c2b, _ = bf01.encrypt_batch(eng, inst.g1x, data, inst.r, ids=inst.ids, msg_off=off)        # host identities and public values beside device messages
    assert same_on_tensors(c1b, inst.c1) and same_on_tensors(c2b, inst.c2_data)
    m, lens = bf01.decrypt_batch(eng, sk, c1, c2, off)
    assert same_on_tensors(m, inst.dec_data) and isinstance(lens, torch.Tensor) and lens.numpy().astype(np.uint32).tolist() == inst.c2_len.tolist()
    m1, _ = bf01.decrypt_batch(eng, sk[0], c1, c2, off)                                    # one key for all, on tensors
    assert isinstance(m1, torch.Tensor) and m1.numpy().tobytes() == bf01.decrypt_batch(MaskStandIn(oracle), inst.sk[0], inst.c1, inst.c2_data, inst.off)[0].tobytes()
    seeded = bf01.encrypt_batch_seeded(eng, g1x, data, rng.Randomness(eng, SEED), qids=qids, msg_off=off)
    plain = MaskStandIn(oracle)
    host = bf01.encrypt_batch_seeded(plain, inst.g1x, inst.data, rng.Randomness(plain, SEED), qids=inst.qids, msg_off=inst.off)
    assert same_on_tensors(seeded[0], host[0]) and same_on_tensors(seeded[1], host[1])
    with pytest.raises(ValueError):
        bf01.encrypt_batch(eng, inst.g1x, data, kbytes(inst.r), qids=qids, msg_off=off)    # host scalars beside device points
