"""Waters05 IBE batches through the host planner gopairingbasedcryptography_amd/waters05.py, on the oracle engine (the same flow runs
on the GPU engine in test_waters05_gpu.py): identity_masks against the reference's Id[] order, then a small seeded instance
(waters05_fixture.py) — keygen_batch and encrypt_batch byte-identical both to the reference's own sequence written out with oracle
calls (the chain of G2Affine.Add over Id[], ScalarMultiplication, Add / Pair, Exp, Mul) and to the fixture's exponent route;
decrypt_batch returns every message and equals the reference's Mul / Div form; a key of another identity does not decrypt."""
import hashlib

import numpy as np
import pytest

from standin_engine import StandInEngine, TensorEngine, same_on_tensors, tensors
from waters05_fixture import Instance, id_bits
from gopairingbasedcryptography_amd import waters05

IDS = ["alice@example.com", "bob@example.com", "carol", "身份", "x"]


@pytest.fixture(scope="module")
def inst(oracle):
    return Instance(oracle, IDS, tag="plan")


def test_identity_masks_are_the_reference_bits():
    m = waters05.identity_masks(IDS)
    assert m.shape == (len(IDS), 32) and m.dtype == np.uint8
    for row, s in zip(m, IDS):
        assert row.tobytes() == hashlib.sha256(s.encode()).digest()
        assert np.unpackbits(row).tolist() == id_bits(s)                       # Id[8 w + t] = bit 7 - t of byte w
    assert (waters05.identity_masks([b"bob@example.com"]) == m[1]).all() and waters05.identity_masks([]).shape == (0, 32)
    with pytest.raises(ValueError):
        waters05.identity_masks(["a", ""])


def test_keygen_and_encrypt_match_the_reference_sequence(oracle, inst):
    eng = StandInEngine(oracle)
    n = len(IDS)
    table = waters05.hash_table(eng, inst.u_prime, inst.ui)
    assert table.nbits == 256 and table.g2 and (table.O == inst.u_prime).all()
    masks = waters05.identity_masks(IDS)
    d1, d2 = waters05.keygen_batch(eng, table, inst.g2_alpha, masks, inst.rows(inst.r))
    c1, c2, c3 = waters05.encrypt_batch(eng, table, inst.e_alpha, inst.messages, masks, inst.rows(inst.t))
    assert table.calls == 2                                                    # one table sum per batch
    assert d1.shape == (n, 128) and d2.shape == (n, 64) and c1.shape == (n, 384) and c2.shape == (n, 64) and c3.shape == (n, 128)
    for j in range(n):
        rd1, rd2 = inst.reference_keygen(j)
        assert (d1[j] == rd1).all() and (d2[j] == rd2).all(), j
        rc1, rc2, rc3 = inst.reference_encrypt(j)
        assert (c1[j] == rc1).all() and (c2[j] == rc2).all() and (c3[j] == rc3).all(), j
    assert (d1 == inst.d1).all() and (d2 == inst.d2).all() and (c1 == inst.c1).all() and (c2 == inst.c2).all() and (c3 == inst.c3).all()
    # Python integers as the randomness give the same bytes
    assert (waters05.keygen_batch(eng, table, inst.g2_alpha, masks, inst.r)[0] == d1).all()
    with pytest.raises(ValueError):
        waters05.keygen_batch(eng, table, inst.g2_alpha, masks, inst.r[:-1])
    with pytest.raises(ValueError):
        waters05.encrypt_batch(eng, table, inst.e_alpha, inst.messages[:-1], masks, inst.t)
    with pytest.raises(ValueError):
        waters05.hash_table(eng, inst.u_prime, inst.ui[:255])


def test_decrypt_returns_the_messages(oracle, inst):
    eng = StandInEngine(oracle)
    n = len(IDS)
    calls = []
    eng.multi_pair = lambda P, Q, off, f=eng.multi_pair: calls.append((len(off) - 1, np.asarray(P).size // 64)) or f(P, Q, off)
    eng.gt_div = eng.gt_inverse = lambda *a: pytest.fail("the quotient folds into the pairing")
    got = waters05.decrypt_batch(eng, (inst.d1, inst.d2), inst.c1, inst.c2, inst.c3)           # key j for ciphertext j
    assert calls == [(n, 2 * n)] and got.shape == (n, 384) and (got == inst.messages).all()
    for j in range(n):
        assert (got[j] == inst.reference_decrypt(inst.d1[j], inst.d2[j], inst.c1[j], inst.c2[j], inst.c3[j])).all(), j
    # one key against every ciphertext: its own decrypts, the others give what the reference's Decrypt gives — not the message
    one = waters05.decrypt_batch(eng, (inst.d1[1], inst.d2[1]), inst.c1, inst.c2, inst.c3)
    assert (one[1] == inst.messages[1]).all()
    for j in (0, 2, 3, 4):
        assert (one[j] != inst.messages[j]).any()
        assert (one[j] == inst.reference_decrypt(inst.d1[1], inst.d2[1], inst.c1[j], inst.c2[j], inst.c3[j])).all(), j
    assert waters05.decrypt_batch(eng, (inst.d1[1], inst.d2[1]), inst.c1[:0], inst.c2[:0], inst.c3[:0]).shape == (0, 384)
    with pytest.raises(ValueError):
        waters05.decrypt_batch(eng, (inst.d1[:2], inst.d2[:2]), inst.c1, inst.c2, inst.c3)
    with pytest.raises(ValueError):
        waters05.decrypt_batch(eng, (inst.d1, inst.d2), inst.c1, inst.c2[:-1], inst.c3)


def test_planner_on_tensors_is_the_planner_on_arrays(oracle, inst):
    """the tensor path on CPU tensors (TensorEngine): the bytes of the numpy run, as tensors"""
    eng = StandInEngine(oracle)
    table = waters05.hash_table(eng, inst.u_prime, inst.ui)
    masks = waters05.identity_masks(IDS[:3])
    tm, tr, tt, tmsg = tensors(masks, inst.rows(inst.r[:3]), inst.rows(inst.t[:3]), inst.messages[:3])
    teng = TensorEngine(eng)
    ttable = TensorEngine(table)
    d1, d2 = waters05.keygen_batch(teng, ttable, inst.g2_alpha, tm, tr)
    assert same_on_tensors(d1, inst.d1[:3]) and same_on_tensors(d2, inst.d2[:3])
    c1, c2, c3 = waters05.encrypt_batch(teng, ttable, inst.e_alpha, tmsg, tm, tt)
    assert same_on_tensors(c1, inst.c1[:3]) and same_on_tensors(c2, inst.c2[:3]) and same_on_tensors(c3, inst.c3[:3])
    assert same_on_tensors(waters05.decrypt_batch(teng, (d1, d2), c1, c2, c3), inst.messages[:3])
    assert same_on_tensors(waters05.decrypt_batch(teng, (inst.d1[0], inst.d2[0]), c1[:1], c2[:1], c3[:1]), inst.messages[:1])   # a host key beside tensors
    with pytest.raises(ValueError):
        waters05.keygen_batch(eng, table, inst.g2_alpha, tm, inst.rows(inst.r[:3]))       # one call, one kind of buffer
    with pytest.raises(ValueError):
        waters05.decrypt_batch(eng, (d1, d2), inst.c1[:3], inst.c2[:3], inst.c3[:3])
