"""Waters11 CP-ABE from boolean formulas through the host planner (gopairingbasedcryptography_amd/formula.py: padded;
waters11.py: encrypt_batch on that block, decrypt_batch_formulas) on the oracle stand-in engine with the formula entries added
(tests/standin_formula.py; the same flow runs on the GPU engine in test_waters11_formula_gpu.py): the block is pad_policies' block of the
restated matrices, Encrypt on it returns the fixture's ciphertext bytes, the 0 / 1 route returns decrypt_batch's messages and ok byte for
byte — the plaintexts where the key satisfies the formula, ok = 0 and a zero row where it does not — and never asks for a field solve, a
negation in Fr or a scalar multiplication."""
import numpy as np
import pytest

import formula_cases as fc
from standin_engine import TensorEngine, recorded, same_on_tensors, tensors
from standin_formula import FormulaStandIn
from sw05_fixture import kbytes
from test_waters11_encrypt_plan import check_ciphertexts, fixture_inputs
from waters11_fixture import Instance
from gopairingbasedcryptography_amd import _buffers as bufs, formula, waters11

KEY = [11, 22, 33, 44]
FORMULAS = [
    ("and", 11, 22),                                                # both held
    ("or", 55, ("and", 33, ("or", 66, 44))),                       # the left child of the root is not held
    11,                                                             # one leaf
    ("and", ("or", 11, 11), ("and", 22, 11)),                      # one attribute on three leaves
    ("and", 11, ("or", 55, 66)),                                    # not satisfied
    ("or", ("and", 11, 55), ("or", ("and", 22, 66), ("and", 33, ("and", 44, 11)))),
    55,                                                             # not satisfied: a single leaf the key lacks
]
FORBIDDEN = ("fr_lsss_weights", "fr_neg", "g1_scalar_mul")
LOGGED = FORBIDDEN + ("fr_lsss_from_formula", "formula_select", "g1_sum_segments", "g1_sub", "multi_pair", "gt_div", "g1_multi_scalar_mul", "fr_lsss_shares")


@pytest.fixture(scope="module")
def setup(oracle):
    eng = FormulaStandIn(oracle)
    policies = [tuple(fc.matrix_of(f)) for f in FORMULAS]
    inst = Instance(eng, KEY, policies)
    return eng, inst, fixture_inputs(inst), formula.encode(FORMULAS)


def scalars(f, n):
    return kbytes(f["s"]).reshape(-1, 32), kbytes([x for r in f["v"] for x in r]).reshape(n, -1, 32), kbytes([x for r in f["r"] for x in r]).reshape(n, -1, 32)


def test_padded_is_the_block_of_the_restated_matrices(setup):
    eng, inst, f, nodes = setup
    want = waters11.pad_policies(inst.policies)
    pad = formula.padded(eng, nodes)
    assert isinstance(pad, waters11.Padded) and (pad.rows, pad.cols) == (want.rows, want.cols) == (7, 5)
    assert np.asarray(pad.matrix).tobytes() == want.matrix.tobytes() and pad.rho.tolist() == want.rho.tolist() and pad.rho.dtype == np.int64
    wide = formula.padded(eng, nodes, rows=8, cols=6)
    assert np.asarray(wide.matrix).tobytes() == waters11.pad_policies(inst.policies, 8, 6).matrix.tobytes() and wide.rho.shape == (len(FORMULAS), 8)
    like = tensors(np.zeros(4, dtype=np.uint8))[0]
    import torch
    on = formula.padded(TensorEngine(eng), torch.from_numpy(nodes.copy()), like=like)
    assert same_on_tensors(on.matrix, want.matrix) and isinstance(on.rho, np.ndarray) and on.rho.tolist() == want.rho.tolist()
    assert bufs.put(on.matrix, like) is on.matrix                                 # a buffer already of the wanted kind passes through
    assert bufs.put(want.matrix, np.zeros(1, np.uint8)) is want.matrix
    none = formula.padded(eng, formula.encode([]))                                # no formulas: an empty block, not an error
    assert np.asarray(none.matrix).shape == (0, 1, 1, 32) and none.rho.shape == (0, 1) and (none.rows, none.cols) == (1, 1)


def test_a_malformed_or_oversized_formula_is_refused_before_the_engine(setup):
    eng, inst, f, nodes = setup
    probe = FormulaStandIn(eng.o)
    calls = recorded(probe, LOGGED)
    bad = nodes.copy()
    bad[2, 1] = 5                                                                 # a code behind the tree's end
    for fn in (lambda: formula.padded(probe, bad), lambda: formula.padded(probe, nodes, rows=6), lambda: formula.padded(probe, nodes, cols=4),
               lambda: formula.padded(probe, nodes, rows=65), lambda: formula.padded(probe, nodes.astype(np.int32))):
        with pytest.raises(ValueError):
            fn()
    assert calls == []


def test_encrypt_on_the_padded_block_returns_the_fixture_ciphertexts(setup):
    eng, inst, f, nodes = setup
    msgs = np.asarray(inst.msgs)
    got = waters11.encrypt_batch(eng, f["g1a"], f["e_alpha"], f["h"], formula.padded(eng, nodes), msgs, f["s"], f["v"], f["r"])
    check_ciphertexts(inst, got)
    tm, ts, tv, tr = tensors(msgs, *scalars(f, inst.n))
    pad = formula.padded(TensorEngine(eng), nodes, like=tm)
    on = waters11.encrypt_batch(TensorEngine(eng), f["g1a"], f["e_alpha"], f["h"], pad, tm, ts, tv, tr)
    assert all(same_on_tensors(g, np.asarray(w)) for g, w in zip(on, got))


def test_decrypt_batch_formulas_is_decrypt_batch_without_a_solve(setup):
    eng, inst, f, nodes = setup
    msgs = np.asarray(inst.msgs).reshape(-1, 384)
    pad = formula.padded(eng, nodes)
    ct = waters11.encrypt_batch(eng, f["g1a"], f["e_alpha"], f["h"], pad, msgs, f["s"], f["v"], f["r"])
    want, want_ok = waters11.decrypt_batch(eng, inst.key, pad, *ct)
    probe = FormulaStandIn(eng.o)
    calls = recorded(probe, LOGGED)
    out, ok = waters11.decrypt_batch_formulas(probe, inst.key, nodes, *ct)
    names = [name for name, _ in calls]
    assert not set(names) & set(FORBIDDEN) and names == ["formula_select", "g1_sum_segments", "g1_sub", "g1_sub", "multi_pair", "gt_div"]
    sat = inst.satisfied()
    assert sat == [True, True, True, True, False, True, False] and ok.tolist() == want_ok.tolist() == [1, 1, 1, 1, 0, 1, 0]
    assert np.asarray(out).tobytes() == np.asarray(want).tobytes()
    for j in range(inst.n):
        assert np.asarray(out)[j].tobytes() == (msgs[j].tobytes() if sat[j] else bytes(384)), j
    # the fixture's own ciphertexts carry random points on the padding rows: they are never chosen
    again, ok2 = waters11.decrypt_batch_formulas(eng, inst.key, nodes, inst.c, inst.c_prime, inst.cx, inst.dx, rows=inst.R)
    assert ok2.tolist() == ok.tolist() and np.asarray(again).tobytes() == np.asarray(out).tobytes()
    # ... and so on tensors, with the codes as a tensor or as the host table
    import torch
    tct = tensors(*ct)
    for codes in (torch.from_numpy(nodes.copy()), nodes):
        on, on_ok = waters11.decrypt_batch_formulas(TensorEngine(eng), inst.key, codes, *tct)
        assert same_on_tensors(on, np.asarray(out)) and on_ok.numpy().tolist() == ok.tolist()


def test_an_unsatisfied_key_and_a_malformed_formula_give_zero_rows(setup):
    eng, inst, f, nodes = setup
    msgs = np.asarray(inst.msgs).reshape(-1, 384)
    ct = waters11.encrypt_batch(eng, f["g1a"], f["e_alpha"], f["h"], formula.padded(eng, nodes), msgs, f["s"], f["v"], f["r"])
    K, L, kx = inst.key
    out, ok = waters11.decrypt_batch_formulas(eng, (K, L, {55: kx[11]}), nodes, *ct)                 # holds 55 alone, with a component that is not its own
    assert ok.tolist() == [0, 1, 0, 0, 0, 0, 1] and not np.asarray(out)[[0, 2, 3, 4, 5]].any()
    out, ok = waters11.decrypt_batch_formulas(eng, (K, L, {}), nodes, *ct)
    assert not ok.any() and not np.asarray(out).any()
    bad = nodes.copy()
    bad[0, 0] = -4
    bad[2, 1] = 5
    out, ok = waters11.decrypt_batch_formulas(eng, inst.key, bad, *ct, rows=7)
    assert ok.tolist() == [0, 1, 0, 1, 0, 1, 0] and not np.asarray(out)[[0, 2]].any() and np.asarray(out)[1].tobytes() == msgs[1].tobytes()
    with pytest.raises(ValueError, match="need c"):
        waters11.decrypt_batch_formulas(eng, inst.key, nodes, *ct, rows=8)
    empty = waters11.decrypt_batch_formulas(eng, inst.key, nodes[:0], ct[0][:0], ct[1][:0], ct[2][:0], ct[3][:0], rows=7)
    assert empty[0].shape == (0, 384) and empty[1].shape == (0,)
