"""The SW05 planners from attribute rows (sw05.decrypt_batch / decrypt_batch_large with ct_attrs as [n, a, 32] scalar rows), CPU part: on the
stand-in engine of tests/standin_engine.py with fr_find_common in Python integers, and behind TensorEngine, against the integer form of the
same planner on the same instance — the bytes must be the same."""
import numpy as np
import pytest

import select_cases as sel
from standin_engine import StandInEngine, TensorEngine, recorded, same_on_tensors, tensors
from sw05_fixture import Instance, kints
from test_sw05_plan import CTS, KEY, cts_for
from gopairingbasedcryptography_amd import sw05

R = sel.R


def RowsEngine(oracle):
    """the stand-in engine with a record of its selections: (key sets, lists, m, a, d) per fr_find_common call"""
    eng = StandInEngine(oracle)
    calls = recorded(eng, ("fr_find_common",))
    eng.selections = lambda: [(np.asarray(sets).size // (32 * m), np.asarray(lists).size // (32 * a), m, a, d) for _, (sets, lists, m, a, d) in calls]
    return eng


def decrypt(eng, inst, d, ct_attrs, large, key=None, parts=None):
    E, e_prime = parts[:2] if parts else (inst.E, inst.e_prime)
    if large:
        return sw05.decrypt_batch_large(eng, key or inst.key, d, ct_attrs, E, parts[2] if parts else inst.e_pp, e_prime)
    return sw05.decrypt_batch(eng, key or inst.key, d, ct_attrs, E, e_prime)


def test_attribute_rows():
    rows = sw05.attribute_rows([1, R + 2, -1])
    assert rows.shape == (3, 32) and rows.dtype == np.uint8 and kints(rows) == [1, 2, R - 1]
    nested = sw05.attribute_rows(cts_for(2))
    assert nested.shape == (4, 5, 32) and kints(nested) == [v % R for c in cts_for(2) for v in c]
    assert sw05.attribute_rows([]).shape == (0, 32)
    with pytest.raises(ValueError):
        sw05.attribute_rows([[1, 2], [3]])


@pytest.mark.parametrize("large", [False, True])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_rows_form_is_the_integer_form(oracle, d, large):
    eng = RowsEngine(oracle)
    cts = cts_for(d)
    inst = Instance(eng, d, KEY, cts, n_univ=5 if large else None, tag="p%d" % d)
    want, want_ok = decrypt(eng, inst, d, cts, large)
    assert want_ok.tolist() == [1, 1, 0, 1] and eng.selections() == []
    rows = sel.rows(v for c in cts for v in c).reshape(4, 5, 32)                                  # unreduced: r - 3 and full-size values as they are
    calls = []
    eng.multi_pair = lambda P, Q, off, f=eng.multi_pair: calls.append((len(off) - 1, np.asarray(P).size // 64)) or f(P, Q, off)
    got, ok = decrypt(eng, inst, d, rows, large)
    assert eng.selections() == [(1, 4, 6, 5, d)] and calls == [(3, 3 * d * (2 if large else 1))]    # one selection; the item below the threshold takes no part
    assert ok.dtype == np.uint8 and ok.tolist() == [1, 1, 0, 1] and got.shape == (4, 384)
    assert got.tobytes() == np.asarray(want).tobytes() and not got[2].any()
    for t in (0, 1, 3):
        assert (got[t] == np.asarray(inst.msgs)[t]).all(), t
    # the key's attributes as rows, and as rows that are equal to the integers only modulo r
    for attrs in (sw05.attribute_rows(KEY), sel.rows([KEY[0] + R, KEY[1] + 2 * R] + [v % R for v in KEY[2:]])):
        again, ok2 = decrypt(eng, inst, d, rows, large, key=(attrs,) + tuple(inst.key[1:]))
        assert again.tobytes() == got.tobytes() and ok2.tolist() == [1, 1, 0, 1]
    # behind TensorEngine: tensors in, tensors out, the same bytes
    parts = tensors(inst.E, inst.e_prime, *([inst.e_pp] if large else []))
    got_t, ok_t = decrypt(TensorEngine(eng), inst, d, tensors(rows)[0], large, parts=parts)
    assert same_on_tensors(got_t, got) and same_on_tensors(ok_t, ok)
    key_t = tuple(tensors(sw05.attribute_rows(KEY), *inst.key[1:]))
    got_t, ok_t = decrypt(TensorEngine(eng), inst, d, tensors(rows)[0], large, key=key_t, parts=parts)
    assert same_on_tensors(got_t, got) and same_on_tensors(ok_t, ok)


@pytest.mark.parametrize("large", [False, True])
def test_a_key_per_item(oracle, large):
    """n (key, ciphertext) pairs whose keys differ — other attributes, other secrets: every pair as the integer form decrypts it alone"""
    eng = RowsEngine(oracle)
    d, cts = 2, cts_for(2)
    other = [17, 2, 50, 9 + R, 51, 4]
    insts = [Instance(eng, d, KEY, cts, n_univ=5 if large else None, tag="ka"), Instance(eng, d, other, cts, n_univ=5 if large else None, tag="kb")]
    pairs = [(0, 0), (1, 1), (0, 2), (1, 3), (1, 0), (0, 3), (1, 2)]                              # (instance, ciphertext)
    want, want_ok = [], []
    for i, t in pairs:
        inst = insts[i]
        parts = [inst.E[t:t + 1], inst.e_prime.reshape(-1, 384)[t:t + 1]] + ([inst.e_pp.reshape(-1, 64)[t:t + 1]] if large else [])
        out, ok = decrypt(eng, inst, d, [cts[t]], large, parts=parts)
        want.append(np.asarray(out).reshape(384))
        want_ok.append(int(ok[0]))
    assert want_ok == [1, 1, 0, 1, 1, 1, 0] and eng.selections() == []              # ciphertext 2 shares one attribute (4) with either key
    stack = lambda f: np.stack([np.asarray(f(insts[i], t)) for i, t in pairs])
    rows = stack(lambda inst, t: sel.rows(cts[t]))
    attrs = stack(lambda inst, t: sel.rows(inst.key[0]))
    key = (attrs,) + tuple(stack(lambda inst, t, c=c: inst.key[c]) for c in range(1, 3 if large else 2))
    parts = [stack(lambda inst, t: inst.E[t]), stack(lambda inst, t: inst.e_prime.reshape(-1, 384)[t])] + ([stack(lambda inst, t: inst.e_pp.reshape(-1, 64)[t])] if large else [])
    got, ok = decrypt(eng, None, d, rows, large, key=key, parts=parts)
    assert eng.selections() == [(7, 7, 6, 5, d)] and ok.tolist() == want_ok
    assert got.tobytes() == np.stack(want).tobytes() and not got[2].any() and not got[6].any()
    assert (got[0] != got[4]).any()                                                               # the keys do differ
    got_t, ok_t = decrypt(TensorEngine(eng), None, d, tensors(rows)[0], large, key=tuple(tensors(*key)), parts=tensors(*parts))
    assert same_on_tensors(got_t, got) and same_on_tensors(ok_t, ok)


def test_rows_form_with_nothing_decryptable_and_bad_shapes(oracle):
    eng = RowsEngine(oracle)
    inst = Instance(eng, 2, KEY, [CTS[2], CTS[4]], tag="none")
    rows = sw05.attribute_rows(inst.ct_attrs)
    eng.multi_pair = eng.g1_scalar_mul = eng.fr_lagrange_basis = lambda *a: pytest.fail("no group operation without a decryptable ciphertext")
    out, ok = sw05.decrypt_batch(eng, inst.key, 2, rows, inst.E, inst.e_prime)
    assert ok.tolist() == [0, 0] and out.shape == (2, 384) and not out.any()
    eng.fr_find_common = lambda *a: pytest.fail("no selection before the shapes are checked")
    out, ok = sw05.decrypt_batch(eng, inst.key, 2, rows[:0], inst.E[:0], inst.e_prime[:0])       # no items
    assert out.shape == (0, 384) and ok.shape == (0,)
    bad = [lambda: sw05.decrypt_batch(eng, inst.key, 2, rows, inst.E[:1], inst.e_prime),
           lambda: sw05.decrypt_batch(eng, inst.key, 0, rows, inst.E, inst.e_prime),
           lambda: sw05.decrypt_batch(eng, inst.key, 2, rows, tensors(inst.E)[0], inst.e_prime),                      # one call, one kind of buffer
           lambda: sw05.decrypt_batch(eng, inst.key, 2, tensors(rows)[0], inst.E, inst.e_prime),
           lambda: sw05.decrypt_batch(eng, (np.zeros((3, 6, 32), np.uint8), inst.key[1]), 2, rows, inst.E, inst.e_prime),      # a key per item needs n keys
           lambda: sw05.decrypt_batch(eng, (np.zeros((6, 31), np.uint8), inst.key[1]), 2, rows, inst.E, inst.e_prime)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
