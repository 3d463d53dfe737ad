"""BSW07 SetUp and KeyGenerate through the host planner (gopairingbasedcryptography_amd/bsw07.py: setup, setup_seeded, keygen_batch,
keygen_batch_seeded, key_for_leaves) on the oracle stand-in engine with the row form of g2_scalar_mul (tests/standin_rows.py; the same
flow runs on the GPU engine in test_bsw07_keygen_gpu.py): setup against Python integers; keygen_batch for 3 users x 4 attributes with
H2(a) = [h_a] g2 byte-equal to the keys tests/bsw07_keys_fixture.py makes from the discrete logs, through ONE row call — A bases, A U
scalars, attribute-major; held zeroes exactly its rows; h2=None is the generator route; the seeded draw order; key_for_leaves on a tree
with a repeated attribute and an attribute the list lacks; the argument errors."""
import numpy as np
import pytest

import bn254_py as o
import chacha_cases as cc
from bsw07_fixture import example_tree, leaves, sc
from bsw07_keys_fixture import user_keys
from standin_engine import TensorEngine, recorded, same_on_tensors, tensors
from standin_rows import RowsStandIn
from sw05_fixture import kbytes
from gopairingbasedcryptography_amd import bsw07, rng

R = o.R
G1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
G2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
SEED = bytes((13 * i + 7) % 256 for i in range(32))
ATTRS = [11, 22, 33, 44]                                                  # the list of the authority: 55, a leaf of the tree, is not on it
SETS = [{11, 22, 33, 44}, {22, 44}, {11}]                                 # what each of the 3 users gets
U, A = len(SETS), len(ATTRS)


def mul(eng, gen, ks):
    fn = eng.g2_scalar_mul if len(gen) == 128 else eng.g1_scalar_mul
    return np.asarray(fn(gen, kbytes([k % R for k in ks]))).reshape(len(ks), -1)


@pytest.fixture(scope="module")
def setup(oracle):
    eng = RowsStandIn(oracle)
    alpha, beta = sc("alpha"), sc("beta")
    pp, msk = bsw07.setup(eng, alpha, beta)
    h2 = mul(eng, G2, [sc("h", a) for a in ATTRS])
    r = [sc("r-user", u) for u in range(U)]
    rj = [[sc("rj-user-%d" % u, a) for a in ATTRS] for u in range(U)]
    held = np.array([[a in s for a in ATTRS] for s in SETS], dtype=np.uint8)
    return eng, pp, msk, h2, r, rj, held


def test_setup_against_python_integers(setup):
    eng, pp, msk, *_ = setup
    alpha, beta = sc("alpha"), sc("beta")
    assert set(pp) == {"h", "f", "e_alpha"} and set(msk) == {"beta", "g2_alpha"}
    assert np.asarray(pp["h"]).tobytes() == mul(eng, G1, [beta]).tobytes() and np.asarray(pp["f"]).tobytes() == mul(eng, G2, [pow(beta, -1, R)]).tobytes()
    assert np.asarray(pp["e_alpha"]).tobytes() == np.asarray(eng.gt_exp(eng.pair_batch(G1, G2), [alpha])).tobytes()
    assert np.asarray(msk["beta"]).tobytes() == kbytes([beta]).tobytes() and np.asarray(msk["g2_alpha"]).tobytes() == mul(eng, G2, [alpha]).tobytes()
    table = eng.GTFixedBase(np.asarray(eng.pair_batch(G1, G2)).reshape(1, 384))
    pp2, msk2 = bsw07.setup(eng, kbytes([alpha]), kbytes([beta]), gt_table=table)
    assert all(np.asarray(pp2[k]).tobytes() == np.asarray(pp[k]).tobytes() for k in pp) and all(np.asarray(msk2[k]).tobytes() == np.asarray(msk[k]).tobytes() for k in msk)
    assert table.calls == [(1, 1, 1)] and not table.closed
    tp, tm = bsw07.setup(TensorEngine(eng), *tensors(kbytes([alpha]), kbytes([beta])))
    assert all(same_on_tensors(tp[k], np.asarray(pp[k])) for k in pp) and all(same_on_tensors(tm[k], np.asarray(msk[k])) for k in msk)
    zero, _ = bsw07.setup(eng, alpha, 0)                                  # fr.Element.Inverse: 0 -> 0, f = the point at infinity
    assert not np.asarray(zero["f"]).any() and not np.asarray(zero["h"]).any()
    with pytest.raises(ValueError):
        bsw07.setup(eng, [alpha, alpha], beta)


def test_keygen_batch_is_one_row_call_and_the_fixtures_keys(setup):
    eng, pp, msk, h2, r, rj, held = setup
    calls = recorded(eng, ["g2_scalar_mul"])
    try:
        D, dj, djp = bsw07.keygen_batch(eng, msk, h2, r, rj, held=held)
    finally:
        del eng.g2_scalar_mul                                             # the instance attribute recorded() set; the method is back
    row_calls = [a for _, a in calls if np.asarray(a[0]).size == A * 128 and np.asarray(a[1]).size == A * U * 32]
    assert len(row_calls) == 1 and len(calls) == 2 and 1 < A < A * U      # the other one is D: a base per scalar
    bases, scalars = row_calls[0]
    assert np.asarray(bases).tobytes() == h2.tobytes()
    assert np.asarray(scalars).tobytes() == kbytes([rj[u][a] for a in range(A) for u in range(U)]).tobytes()        # attribute-major
    assert D.shape == (U, 128) and dj.shape == djp.shape == (U, A, 128)
    # the fixture's keys, from the discrete logs, in the leaf order of the tree
    tree = example_tree()
    bsw07.assign_leaf_ids(tree)
    wD, wdj, wdjp, _, _ = user_keys(eng, tree, SETS)
    lheld, ldj, ldjp = bsw07.key_for_leaves(tree, ATTRS, held, dj, djp)
    attrs_of_leaves = [l.attribute for l in leaves(tree)]
    assert np.asarray(D).tobytes() == wD.tobytes()
    assert lheld.tolist() == [[int(a in s) for a in attrs_of_leaves] for s in SETS] == bsw07.leaf_mask(tree, SETS).tolist()
    for u in range(U):
        for y, a in enumerate(attrs_of_leaves):
            if a in SETS[u]:
                assert ldj[u, y].tobytes() == wdj[u, y].tobytes() and ldjp[u, y].tobytes() == wdjp[u, y].tobytes(), (u, y)
            else:
                assert not ldj[u, y].any() and not ldjp[u, y].any(), (u, y)
    # held zeroes exactly its rows
    full = bsw07.keygen_batch(eng, msk, h2, r, rj)
    assert np.asarray(full[0]).tobytes() == np.asarray(D).tobytes()
    for u in range(U):
        for a in range(A):
            for got, whole in ((dj, full[1]), (djp, full[2])):
                assert got[u, a].tobytes() == (whole[u, a].tobytes() if held[u, a] else bytes(128)) and whole[u, a].any(), (u, a)
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(bsw07.keygen_batch(eng, msk, h2, r, rj, held=held.astype(bool).tolist()), (D, dj, djp)))
    targs = tensors(h2, kbytes(r).reshape(-1, 32), kbytes(sum(rj, [])).reshape(U, A, 32), held)
    assert all(same_on_tensors(t, np.asarray(w)) for t, w in zip(bsw07.keygen_batch(TensorEngine(eng), msk, *targs), (D, dj, djp)))       # the master key from the host
    tk = bsw07.keygen_batch(TensorEngine(eng), {k: tensors(v)[0] for k, v in msk.items()}, *tensors(h2, kbytes(r).reshape(-1, 32), kbytes(sum(rj, [])).reshape(U, A, 32), held))
    assert all(same_on_tensors(t, np.asarray(w)) for t, w in zip(tk, (D, dj, djp)))


def test_no_hash_is_the_generator_route(setup):
    eng, pp, msk, h2, r, rj, held = setup
    calls = recorded(eng, ["g2_scalar_mul"])
    try:
        ref = bsw07.keygen_batch(eng, msk, None, r, rj)
    finally:
        del eng.g2_scalar_mul
    assert len(calls) == 1                                                # D only: no variable-base row call
    gen = bsw07.keygen_batch(eng, msk, np.tile(G2, (A, 1)), r, rj)
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(ref, gen))
    want = mul(eng, G2, [r[u] + rj[u][a] for u in range(U) for a in range(A)])
    assert np.asarray(ref[1]).tobytes() == want.tobytes()


def test_seeded_forms_draw_in_the_documented_order(setup):
    eng, pp, msk, h2, *_ = setup
    eng.draws.clear()
    rs = rng.Randomness(eng, SEED)
    got = bsw07.keygen_batch_seeded(eng, msk, h2, U, rs)
    assert eng.draws == [(U, 0, 0), (U * A, 1, 0)] and rs.next_stream == 2                # r [U], then rj [U, A]
    want = bsw07.keygen_batch(eng, msk, h2, cc.scalars(SEED, 0, 0, U), cc.scalars(SEED, 1, 0, U * A).reshape(U, A, 32))
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(got, want))
    again = bsw07.keygen_batch_seeded(eng, msk, h2, U, rng.Randomness(eng, SEED))
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(got, again))
    none = bsw07.keygen_batch_seeded(eng, msk, None, U, rng.Randomness(eng, SEED), n_attrs=A)
    assert np.asarray(none[0]).tobytes() == np.asarray(got[0]).tobytes() and none[1].shape == (U, A, 128)
    eng.draws.clear()
    rs = rng.Randomness(eng, SEED)
    spp, smsk = bsw07.setup_seeded(eng, rs)
    assert eng.draws == [(1, 0, 0), (1, 1, 0)] and rs.next_stream == 2                    # alpha, then beta
    wpp, wmsk = bsw07.setup(eng, cc.scalars(SEED, 0, 0, 1), cc.scalars(SEED, 1, 0, 1))
    assert all(np.asarray(spp[k]).tobytes() == np.asarray(wpp[k]).tobytes() for k in wpp) and all(np.asarray(smsk[k]).tobytes() == np.asarray(wmsk[k]).tobytes() for k in wmsk)


def test_key_for_leaves_repeats_and_pads(setup):
    eng, pp, msk, h2, r, rj, held = setup
    tree = example_tree()                                                 # leaves 11, 22, 33, 44, 55, 11: 11 twice, 55 not on the list
    dj = np.arange(U * A * 128, dtype=np.uint32).astype(np.uint8).reshape(U, A, 128) | 1
    djp = dj ^ 0x80
    lheld, ldj, ldjp = bsw07.key_for_leaves(tree, ATTRS, None, dj, djp)
    assert lheld.shape == (U, 6) and ldj.shape == ldjp.shape == (U, 6, 128)
    assert lheld.tolist() == [[1, 1, 1, 1, 0, 1]] * U
    for y, col in enumerate([0, 1, 2, 3, None, 0]):
        assert ldj[:, y].tobytes() == (dj[:, col].tobytes() if col is not None else bytes(U * 128))
        assert ldjp[:, y].tobytes() == (djp[:, col].tobytes() if col is not None else bytes(U * 128))
    plan = bsw07.share_plan(tree)
    masked = bsw07.key_for_leaves(plan, ATTRS, held, dj, djp)
    assert masked[0].tolist() == [[1, 1, 1, 1, 0, 1], [0, 1, 0, 1, 0, 0], [1, 0, 0, 0, 0, 1]]
    assert not masked[1][1, 0].any() and masked[1][2, 5].tobytes() == dj[2, 0].tobytes()
    tl = bsw07.key_for_leaves(plan, ATTRS, *tensors(held, dj, djp))
    assert all(same_on_tensors(t, np.asarray(w)) for t, w in zip(tl, masked))


def test_argument_errors(setup):
    eng, pp, msk, h2, r, rj, held = setup
    dj = np.zeros((U, A, 128), dtype=np.uint8)
    for bad in (lambda: bsw07.keygen_batch(eng, msk, h2, r, rj[:-1]), lambda: bsw07.keygen_batch(eng, msk, h2[:-1], r, rj),
                lambda: bsw07.keygen_batch(eng, msk, h2.reshape(-1)[:-1], r, rj), lambda: bsw07.keygen_batch(eng, msk, h2, r, rj, held=held[:-1]),
                lambda: bsw07.keygen_batch(eng, {"beta": msk["beta"], "g2_alpha": h2}, h2, r, rj),
                lambda: bsw07.key_for_leaves(example_tree(), ATTRS + [11], None, dj, dj), lambda: bsw07.key_for_leaves(example_tree(), ATTRS[:-1], None, dj, dj[:, :-1]),
                lambda: bsw07.key_for_leaves(example_tree(), ATTRS, held[:-1], dj, dj), lambda: bsw07.key_for_leaves(example_tree(), [], None, dj, dj)):
        with pytest.raises(ValueError):
            bad()
    empty = bsw07.keygen_batch(eng, msk, h2, [], [])
    assert empty[0].shape == (0, 128) and empty[1].shape == empty[2].shape == (0, A, 128)
