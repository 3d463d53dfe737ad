"""The seeded planners (bsw07.encrypt_batch_seeded, sw05.keygen_batch_seeded / keygen_batch_large_seeded, waters11.encrypt_batch_seeded,
lw11.encrypt_batch_seeded) and rng.Randomness on the oracle stand-in engine (tests/standin_engine.py), whose fr_random here is the
Python oracle of tests/chacha_cases.py: each returns, byte for byte, what the existing planner returns on the oracle's scalars of the
documented streams in the documented order; a second call on one Randomness takes later streams and gives other ciphertexts; a draw of
no columns takes no stream.  The same flow runs on the GPU engine in test_seeded_gpu.py."""
import numpy as np
import pytest

import chacha_cases as cc
from bsw07_fixture import Instance as Bsw07Instance, example_tree
from lw11_fixture import Instance as Lw11Instance, and_or_policy
from standin_engine import StandInEngine, StandInFixedBase, TensorEngine, same_on_tensors, tensors
from waters11_fixture import Instance as Waters11Instance, small_policies
from test_bsw07_encrypt_plan import fixture_inputs as bsw07_inputs
from test_lw11_encrypt_plan import fixture_inputs as lw11_inputs
from test_sw05_keygen_plan import instance as sw05_instance, three_users
from test_waters11_encrypt_plan import fixture_inputs as waters11_inputs
import share_cases as sc
from gopairingbasedcryptography_amd import bsw07, lw11, rng, sw05, waters11

SEED = bytes((7 * i + 3) % 256 for i in range(32))


class SeededStandIn(StandInEngine):
    """the stand-in engine with fr_random from the oracle; every draw is written down as (n, stream, first)"""

    def __init__(self, oracle):
        super().__init__(oracle)
        self.draws = []

    def fr_random(self, seed, n, stream=0, first=0, out=None, like=None):
        self.draws.append((n, stream, first))
        return cc.scalars(bytes(seed), stream, first, n)


def drawn(stream, *shape):
    """the oracle's scalars of one draw: [*shape, 32] from index 0 of `stream`, row-major"""
    return cc.scalars(SEED, stream, 0, int(np.prod(shape))).reshape(*shape, 32)


def same(got, want):
    return len(got) == len(want) and all(np.asarray(g).shape == np.asarray(w).shape and np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ BSW07
@pytest.fixture(scope="module")
def bsw(oracle):
    eng = SeededStandIn(oracle)
    inst = Bsw07Instance(eng, example_tree(), user_attrs=[11, 22, 33, 99], n_ct=3)
    _, _, h, h1 = bsw07_inputs(inst, 3)
    return eng, inst, h, h1, np.stack(inst.msgs)


def test_bsw07_seeded_is_encrypt_batch_on_the_drawn_scalars(bsw):
    eng, inst, h, h1, msgs = bsw
    C = sc.n_coeffs(inst.tree)
    assert C == 2
    eng.draws.clear()
    r = rng.Randomness(eng, SEED)
    got = bsw07.encrypt_batch_seeded(eng, inst.tree, h, inst.e_alpha, h1, msgs, r)
    assert eng.draws == [(3, 0, 0), (3 * C, 1, 0)] and r.next_stream == 2                          # s [n], then coeffs [n, C]
    assert same(got, bsw07.encrypt_batch(eng, inst.tree, h, inst.e_alpha, h1, msgs, drawn(0, 3), drawn(1, 3, C)))
    again = bsw07.encrypt_batch_seeded(eng, bsw07.share_plan(inst.tree), h, inst.e_alpha, h1, msgs, r, tables=True)
    assert eng.draws[2:] == [(3, 2, 0), (3 * C, 3, 0)] and r.next_stream == 4                      # a second call: later streams, other ciphertexts
    assert same(again, bsw07.encrypt_batch(eng, inst.tree, h, inst.e_alpha, h1, msgs, drawn(2, 3), drawn(3, 3, C)))
    assert all(np.asarray(a).tobytes() != np.asarray(b).tobytes() for a, b in zip(again, got))
    fresh = bsw07.encrypt_batch_seeded(eng, inst.tree, h, inst.e_alpha, h1, msgs, rng.Randomness(eng, SEED), tables=True)
    assert same(fresh, got)                                                                        # reproducible from the seed; tables: the same bytes


def test_bsw07_seeded_single_leaf_draws_s_alone_and_tensors_follow(bsw):
    eng, inst, h, h1, msgs = bsw
    eng.draws.clear()
    r = rng.Randomness(eng, SEED)
    one = bsw07.encrypt_batch_seeded(eng, bsw07.Leaf(11), h, inst.e_alpha, h1, msgs, r)
    assert eng.draws == [(3, 0, 0)] and r.next_stream == 1                                         # C == 0: no stream for the coefficients
    assert same(one, bsw07.encrypt_batch(eng, bsw07.Leaf(11), h, inst.e_alpha, h1, msgs, drawn(0, 3), None))
    none = bsw07.encrypt_batch_seeded(eng, inst.tree, h, inst.e_alpha, h1, msgs[:0], r)
    assert r.next_stream == 1 and [g.shape[0] for g in none] == [0, 0, 0, 0]                       # no ciphertexts: no stream at all
    want = bsw07.encrypt_batch_seeded(eng, inst.tree, h, inst.e_alpha, h1, msgs, rng.Randomness(eng, SEED))
    teng = TensorEngine(eng)
    got = bsw07.encrypt_batch_seeded(teng, inst.tree, h, inst.e_alpha, h1, tensors(msgs)[0], rng.Randomness(teng, SEED))
    assert all(same_on_tensors(g, np.asarray(w)) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ Waters11
@pytest.fixture(scope="module")
def w11(oracle):
    eng = SeededStandIn(oracle)
    policies, key_attrs = small_policies()
    inst = Waters11Instance(eng, key_attrs, policies)
    return eng, inst, waters11_inputs(inst)


def test_waters11_seeded_is_encrypt_batch_on_the_drawn_scalars(w11):
    eng, inst, f = w11
    msgs = np.asarray(inst.msgs)
    pad = waters11.pad_policies(inst.policies)
    n, R, C = inst.n, pad.rows, pad.cols
    assert C > 1
    eng.draws.clear()
    r = rng.Randomness(eng, SEED)
    got = waters11.encrypt_batch_seeded(eng, f["g1a"], f["e_alpha"], f["h"], inst.policies, msgs, r)
    assert eng.draws == [(n, 0, 0), (n * (C - 1), 1, 0), (n * R, 2, 0)] and r.next_stream == 3     # s, v [n, C - 1], r [n, R]
    assert same(got, waters11.encrypt_batch(eng, f["g1a"], f["e_alpha"], f["h"], pad, msgs, drawn(0, n), drawn(1, n, C - 1), drawn(2, n, R)))
    table = waters11.encrypt_table(eng, f["g1a"], f["h"])
    again = waters11.encrypt_batch_seeded(eng, f["g1a"], f["e_alpha"], f["h"], pad, msgs, r, table=table)
    assert [d[1] for d in eng.draws[3:]] == [3, 4, 5] and not table.closed and table.calls == 1
    assert same(again, waters11.encrypt_batch(eng, f["g1a"], f["e_alpha"], f["h"], pad, msgs, drawn(3, n), drawn(4, n, C - 1), drawn(5, n, R)))
    assert all(np.asarray(a).tobytes() != np.asarray(b).tobytes() for a, b in zip(again, got))
    out, ok = waters11.decrypt_batch(eng, inst.key, inst.policies, *got)
    assert ok.tolist() == [1, 1, 1, 0] and np.asarray(out)[:3].tobytes() == msgs.reshape(-1, 384)[:3].tobytes()


def test_waters11_seeded_one_column_draws_no_v(w11):
    eng, inst, f = w11
    u = sorted(f["h"])[0]
    policies = [([[1]], [u]), ([[1], [1]], [u, u])]
    msgs = np.asarray(inst.msgs).reshape(-1, 384)[:2]
    eng.draws.clear()
    r = rng.Randomness(eng, SEED)
    got = waters11.encrypt_batch_seeded(eng, f["g1a"], f["e_alpha"], f["h"], policies, msgs, r)
    assert eng.draws == [(2, 0, 0), (4, 1, 0)] and r.next_stream == 2                              # C == 1: s, then r
    assert same(got, waters11.encrypt_batch(eng, f["g1a"], f["e_alpha"], f["h"], policies, msgs, drawn(0, 2), None, drawn(1, 2, 2)))


# ------------------------------------------------------------------------------------------------ LW11
@pytest.fixture(scope="module")
def lw(oracle):
    eng = SeededStandIn(oracle)
    m, rho = and_or_policy()
    inst = Lw11Instance(eng, m, rho, [11, 22, 44, 99], n_ct=3)
    return eng, inst, lw11_inputs(inst)


def test_lw11_seeded_is_encrypt_batch_on_the_drawn_scalars(lw):
    eng, inst, f = lw
    msgs = np.asarray(inst.msgs)
    n, R, C = inst.n, inst.R, len(inst.matrix[0])
    assert C > 1
    pub = (f["e"], f["egg_alpha"], f["g2_y"], inst.matrix, inst.rho, msgs)
    eng.draws.clear()
    r = rng.Randomness(eng, SEED)
    got = lw11.encrypt_batch_seeded(eng, *pub, r)
    assert eng.draws == [(n, 0, 0), (n * (C - 1), 1, 0), (n * (C - 1), 2, 0), (n * R, 3, 0)] and r.next_stream == 4        # s, v, w, r
    assert same(got, lw11.encrypt_batch(eng, *pub, drawn(0, n), drawn(1, n, C - 1), drawn(2, n, C - 1), drawn(3, n, R)))
    again = lw11.encrypt_batch_seeded(eng, *pub, r)
    assert [d[1] for d in eng.draws[4:]] == [4, 5, 6, 7]
    assert same(again, lw11.encrypt_batch(eng, *pub, drawn(4, n), drawn(5, n, C - 1), drawn(6, n, C - 1), drawn(7, n, R)))
    assert all(np.asarray(a).tobytes() != np.asarray(b).tobytes() for a, b in zip(again, got))
    rows, w = lw11.reconstruction_weights(inst.matrix, inst.rho, inst.user_attrs)
    out = lw11.decrypt_batch(eng, lw11.fold_key(eng, rows, w, inst.h_gid, inst.k_by_row), *got)
    assert np.asarray(out).tobytes() == msgs.tobytes()


def test_lw11_seeded_one_column_draws_neither_v_nor_w(lw):
    eng, inst, f = lw
    a, b = inst.rho[0], inst.rho[1]
    pub = (f["e"], f["egg_alpha"], f["g2_y"], [[1], [1]], [a, b], np.asarray(inst.msgs))
    eng.draws.clear()
    r = rng.Randomness(eng, SEED)
    got = lw11.encrypt_batch_seeded(eng, *pub, r)
    assert eng.draws == [(inst.n, 0, 0), (inst.n * 2, 1, 0)] and r.next_stream == 2
    assert same(got, lw11.encrypt_batch(eng, *pub, drawn(0, inst.n), None, None, drawn(1, inst.n, 2)))


# ------------------------------------------------------------------------------------------------ SW05
def test_sw05_seeded_keys_are_keygen_on_the_drawn_coefficients(oracle):
    eng = SeededStandIn(oracle)
    inst = sw05_instance(eng, 2, 3)
    table = StandInFixedBase(oracle, inst.table_bases, g2=True)
    attrs, _, side = three_users(3)
    y, d = 123456789, 3
    r = rng.Randomness(eng, SEED)
    D = sw05.keygen_batch_seeded(eng, y, d, attrs, side, r)
    assert eng.draws == [(3 * (d - 1), 0, 0)] and r.next_stream == 1                               # coeffs [k, d - 1]
    assert D.tobytes() == sw05.keygen_batch(eng, y, drawn(0, 3, d - 1), attrs, side).tobytes()
    dl, Dl = sw05.keygen_batch_large_seeded(eng, table, 3, y, d, attrs, r)
    assert eng.draws[1:] == [(3 * (d - 1), 1, 0), (3 * 4, 2, 0)] and r.next_stream == 3            # coeffs, then r [k, m]
    assert same((dl, Dl), sw05.keygen_batch_large(eng, table, 3, y, drawn(1, 3, d - 1), attrs, drawn(2, 3, 4)))
    assert D.tobytes() != sw05.keygen_batch_seeded(eng, y, d, attrs, side, r).tobytes() and r.next_stream == 4
    eng.draws.clear()
    one = sw05.keygen_batch_seeded(eng, y, 1, attrs, side, r)                                      # d == 1: nothing to draw
    assert eng.draws == [] and r.next_stream == 4 and one.tobytes() == sw05.keygen_batch(eng, y, None, attrs, side).tobytes()
    l1 = sw05.keygen_batch_large_seeded(eng, table, 3, y, 1, attrs, r)
    assert eng.draws == [(12, 4, 0)] and same(l1, sw05.keygen_batch_large(eng, table, 3, y, None, attrs, drawn(4, 3, 4)))
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="d must be"):
            sw05.keygen_batch_seeded(eng, y, bad, attrs, side, r)
    assert r.next_stream == 5
