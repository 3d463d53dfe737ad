"""BSW07 Encrypt with tables=True through the host planner (gopairingbasedcryptography_amd/bsw07.py: encrypt_batch) on the oracle
stand-in engine (tests/standin_engine.py; the same flow runs on the GPU engine in test_lsss_encrypt_gpu.py): Cy' from a fixed-base
table over the L points of h1 with the L index rows repeating per ciphertext is the fixture's ciphertext, byte for byte what the
default route returns, and the default route does not touch a table."""
import numpy as np
import pytest

import share_cases as sc
from bsw07_fixture import Instance, example_tree
from standin_engine import StandInEngine, TensorEngine, same_on_tensors, tensors
from test_bsw07_encrypt_plan import fixture_arrays, fixture_inputs
from gopairingbasedcryptography_amd import bsw07


@pytest.fixture(scope="module")
def setup(oracle):
    eng = StandInEngine(oracle)
    inst = Instance(eng, example_tree(), user_attrs=[11, 22, 33, 99], n_ct=3)
    return eng, inst, fixture_inputs(inst, 3)


def test_tables_route_returns_the_fixture_ciphertexts(setup):
    eng, inst, (s, coeffs, h, h1) = setup
    msgs = np.stack(inst.msgs)
    before = len(eng.tables)
    plain = bsw07.encrypt_batch(eng, inst.tree, h, inst.e_alpha, h1, msgs, s, coeffs)
    assert len(eng.tables) == before                                                  # the default route is the one it was
    got = bsw07.encrypt_batch(eng, inst.tree, h, inst.e_alpha, h1, msgs, s, coeffs, tables=True)
    assert len(eng.tables) == before + 1 and eng.tables[-1].closed and eng.tables[-1].nbase == 6 and eng.tables[-1].calls == 1
    for g, p, w, shape in zip(got, plain, fixture_arrays(inst), ((3, 384), (3, 64), (3, 6, 64), (3, 6, 64))):
        assert g.shape == shape and g.tobytes() == w.tobytes() == p.tobytes()


def test_tables_route_on_tensors_and_single_leaf(setup):
    eng, inst, (s, coeffs, h, h1) = setup
    msgs = np.stack(inst.msgs)
    want = bsw07.encrypt_batch(eng, inst.tree, h, inst.e_alpha, h1, msgs, s, coeffs)
    tm, ts, tq = tensors(msgs, sc.rows(s).reshape(3, 32), sc.rows([v for q in coeffs for v in q]).reshape(3, -1, 32))
    got = bsw07.encrypt_batch(TensorEngine(eng), inst.tree, h, inst.e_alpha, h1, tm, ts, tq, tables=True)
    assert all(same_on_tensors(g, w) for g, w in zip(got, want))
    one = bsw07.encrypt_batch(eng, bsw07.Leaf(11), h, inst.e_alpha, h1, msgs, s, None, tables=True)
    ref = bsw07.encrypt_batch(eng, bsw07.Leaf(11), h, inst.e_alpha, h1, msgs, s, None)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, ref)) and one[3].shape == (3, 1, 64)


def test_decrypt_of_the_tables_batch_returns_the_messages(setup):
    import bn254_py as o
    eng, inst, (s, coeffs, h, h1) = setup
    eng.g2_neg = lambda q: np.frombuffer(o.g2_to_bytes(o.g2_neg(o.g2_from_bytes(np.asarray(q, dtype=np.uint8).tobytes()))), dtype=np.uint8)
    eng.multi_pair_fixed_q = lambda P, Q: eng.multi_pair(P, np.tile(np.asarray(Q).reshape(-1), 3), np.arange(0, 3 * (np.asarray(Q).size // 128) + 1, np.asarray(Q).size // 128, dtype=np.uint64))
    c_tilde, c, cy, cy_prime = bsw07.encrypt_batch(eng, inst.tree, h, inst.e_alpha, h1, np.stack(inst.msgs), s, coeffs, tables=True)
    folded = bsw07.fold_key(eng, bsw07.decrypt_plan(inst.tree, inst.user_attrs), inst.dj, inst.dj_prime)
    cols = [i - 1 for i in folded[0]]
    out = bsw07.decrypt_batch_arrays(eng, folded, inst.D, c_tilde, c, cy[:, cols], cy_prime[:, cols])
    assert np.asarray(out).tobytes() == np.stack(inst.msgs).tobytes()
