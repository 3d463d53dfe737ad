"""AFP25 KeyGen / Encrypt / ComputeKey (gopairingbasedcryptography_amd/afp25.py: tau_powers, keygen, keygen_seeded, encrypt_tables,
label_points, label_bases, encrypt_batch, encrypt_batch_seeded, compute_key_batch) over the stand-in engine of tests/standin_afp25.py,
without a GPU, on arrays and on CPU tensors.  Every output is held against tests/afp25_scheme_cases.py — the scheme's equations in
scalars, evaluated with the oracle; every pair of routes gives the same bytes; the seeded forms are the plain forms on a second Randomness
of the same seed and take the documented streams; tau_powers makes at most ceil(log2 B) + 1 fr_mul calls and no other scalar work; every
refusal comes before the first engine call; and keygen -> srs_table -> encrypt_batch -> digests_ragged -> compute_key_batch ->
decrypt_batches_ragged returns the messages."""
import math

import numpy as np
import pytest

import afp25_scheme_cases as cases
from afp25_scheme_cases import G1, R
from standin_afp25 import SchemeStandIn, Untouchable
from standin_engine import TensorEngine, recorded, same_on_tensors, tensors
from sw05_fixture import kbytes, kints
from gopairingbasedcryptography_amd import afp25
from gopairingbasedcryptography_amd.rng import Randomness

SEED = bytes(range(32))
SCALAR_ENTRIES = ["fr_mul", "fr_add", "fr_sub", "fr_neg", "fr_inverse", "fr_to_bytes", "fr_poly_from_roots_segments"]


@pytest.fixture(scope="module")
def eng(oracle):
    return SchemeStandIn(oracle)


@pytest.fixture(scope="module")
def b4(oracle):
    return cases.case(oracle, "b4")


def same(got, want):
    return np.asarray(got).shape == np.asarray(want).shape and np.asarray(got).tobytes() == np.asarray(want).tobytes()


def encrypt(eng, c, **kw):
    return afp25.encrypt_batch(eng, c.mpk, c.messages, c.ids, c.r1, c.r2, c.points, c.label_of if c.k > 1 else None, **kw)


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 64, 65])
def test_tau_powers_by_doubling(oracle, B):
    eng = SchemeStandIn(oracle)
    calls = recorded(eng, SCALAR_ENTRIES)
    tau = cases.sc("powers-tau") + R                                           # not canonical going in, canonical coming out
    got = afp25.tau_powers(eng, np.frombuffer(tau.to_bytes(32, "little"), dtype=np.uint8), B)
    assert got.shape == (B, 32) and kints(got) == [pow(tau, i, R) for i in range(1, B + 1)]
    assert {name for name, _ in calls} == {"fr_mul"} and len(calls) <= math.ceil(math.log2(B)) + 1
    assert all(len(a[1]) == 32 for _, a in calls)                              # the second operand is ONE row every time
    tt, = tensors(np.frombuffer(tau.to_bytes(32, "little"), dtype=np.uint8))
    assert same_on_tensors(afp25.tau_powers(TensorEngine(eng), tt, B), got) and same(afp25.tau_powers(eng, tau, B), got)


@pytest.mark.parametrize("name", ["b4", "b65", "b1"])
def test_keygen_is_the_equations(oracle, eng, name):
    c = cases.case(oracle, name)
    mpk = afp25.keygen(eng, c.B, c.tau, c.msk)
    assert sorted(mpk) == ["G1ExpTauPowers", "G2ExpMsk", "G2ExpTau"] and mpk["G1ExpTauPowers"].shape == (c.B, 64)
    assert all(isinstance(v, np.ndarray) and same(v, c.mpk[k]) for k, v in mpk.items())
    rows = tensors(kbytes([c.tau]), kbytes([c.msk]))
    on_tensors = afp25.keygen(TensorEngine(eng), c.B, *rows)
    assert all(same(v, c.mpk[k]) for k, v in on_tensors.items())
    table = afp25.srs_table(eng, G1, mpk["G1ExpTauPowers"])                    # the existing entry keeps working on it
    assert table.nbase == c.B + 1 and same(table.bases[1:], c.mpk["G1ExpTauPowers"])


def test_keygen_refusals_and_the_seeded_form(eng):
    for bad in (0, 1025, -1, True, 2.0):
        with pytest.raises(ValueError, match="invalid B"):
            afp25.keygen(Untouchable(), bad, 1, 2)
        with pytest.raises(ValueError, match="invalid B"):
            afp25.tau_powers(Untouchable(), 1, bad)
        with pytest.raises(ValueError, match="invalid B"):
            afp25.keygen_seeded(Untouchable(), bad, Randomness(Untouchable(), SEED))
    # ONE draw of two scalars, msk then tau
    del eng.draws[:]
    rng = Randomness(eng, SEED)
    mpk, msk = afp25.keygen_seeded(eng, 3, rng)
    assert eng.draws == [(2, 0, 0)] and rng.next_stream == 1 and isinstance(msk, np.ndarray) and msk.shape == (32,)
    want_msk, want_tau = kints(Randomness(eng, SEED).scalars(np.zeros(0, np.uint8), 2))
    assert kints(msk) == [want_msk]
    again = afp25.keygen(eng, 3, want_tau, want_msk)
    assert sorted(mpk) == sorted(again) and all(same(mpk[k], again[k]) for k in again)
    like, = tensors(np.zeros(0, np.uint8))
    tmpk, tmsk = afp25.keygen_seeded(TensorEngine(eng), 3, Randomness(TensorEngine(eng), SEED), like=like)
    assert same_on_tensors(tmsk, msk) and all(same(tmpk[k], again[k]) for k in again)


def test_label_points_and_bases(oracle, eng, b4):
    pts = afp25.label_points(eng, b4.labels)
    assert same(pts, b4.points)
    data = np.frombuffer(b"".join(b4.labels), dtype=np.uint8)
    off = np.cumsum([0] + [len(t) for t in b4.labels]).astype(np.uint64)
    assert same(afp25.label_points(eng, data, off), b4.points)
    bases = afp25.label_bases(eng, b4.mpk, pts)
    e_h = np.asarray(oracle.pair_batch(b4.points, np.tile(cases.G2, (b4.k, 1)))).reshape(b4.k, 384)
    want = np.asarray(oracle.gt_exp(e_h, kbytes([-b4.msk % R] * b4.k)))         # e(h, g2)^(-msk) = e(h, [msk]_2)^-1
    assert same(bases, want)
    assert same_on_tensors(afp25.label_bases(TensorEngine(eng), b4.mpk, tensors(pts)[0]), want)
    assert afp25.label_bases(Untouchable(), b4.mpk, np.zeros((0, 64), np.uint8)).shape == (0, 384)


@pytest.mark.parametrize("name", ["b4", "b65", "b1"])
def test_encrypt_is_the_equations_on_every_route(oracle, name):
    c, eng = cases.case(oracle, name), SchemeStandIn(oracle)
    calls = recorded(eng, ["g2_scalar_mul_base", "g2_scalar_mul", "g2_sub", "g2_add", "g1_scalar_mul", "multi_pair_fixed_q", "gt_inverse", "gt_exp", "gt_mul", "fr_mul", "fr_neg"])
    C1, C2 = encrypt(eng, c)
    assert C1.shape == (c.n, 3, 128) and C2.shape == (c.n, 384)
    assert same(C1, c.C1) and same(C2, c.C2)
    # the reference's operations in the reference's order, then the labels' pairing, its inverse, the power and the product
    assert [n for n, _ in calls] == ["g2_scalar_mul_base", "g2_sub", "g2_scalar_mul", "g2_scalar_mul", "g2_add", "g2_scalar_mul", "g2_scalar_mul",
                                     "multi_pair_fixed_q", "gt_inverse", "gt_exp", "gt_mul"]
    if name == "b4":
        assert not C1[2, 1].any() and not C1[6, 2].any() and same(C2[6], c.messages[6])       # id = tau; r2 = 0
    tables = afp25.encrypt_tables(eng, c.mpk)
    assert tables.g2 and tables.nbase == 3 and same(tables.bases, np.stack([cases.G2, c.mpk["G2ExpMsk"], c.mpk["G2ExpTau"]]))
    bases = afp25.label_bases(eng, c.mpk, c.points)
    gt_table = eng.GTFixedBase(bases) if name != "b65" else None               # the stand-in's GT powers are Python integers: the small cases
    del calls[:]
    fast = encrypt(eng, c, tables=tables, bases=bases)
    assert same(fast[0], c.C1) and same(fast[1], c.C2) and tables.calls == 3
    assert not {"g2_scalar_mul", "g2_scalar_mul_base", "multi_pair_fixed_q", "gt_inverse"} & {n for n, _ in calls}
    del calls[:]
    items = encrypt(eng, c, tables=tables, route="items")
    assert same(items[0], c.C1) and same(items[1], c.C2)
    assert [n for n, _ in calls if n not in ("fr_mul", "fr_neg")] == ["g1_scalar_mul", "multi_pair_fixed_q", "gt_mul"]
    if gt_table is not None:
        del calls[:]
        tabled = encrypt(eng, c, gt_table=gt_table)
        assert same(tabled[0], c.C1) and same(tabled[1], c.C2) and gt_table.calls == [(c.n, 1, c.n if c.k > 1 else 1)]
        assert not {"gt_exp", "multi_pair_fixed_q", "gt_inverse"} & {n for n, _ in calls}
    # CPU tensors through the same planner: every route, the same bytes
    teng = TensorEngine(eng)
    tm, ti, ta, tb, tp, tbases = tensors(c.messages, kbytes(c.ids), kbytes(c.r1), kbytes(c.r2), c.points, bases)
    label_of = c.label_of if c.k > 1 else None
    for kw in (dict(), dict(tables=tables, bases=tbases), dict(route="items")) + ((dict(gt_table=gt_table),) if gt_table is not None else ()):
        got = afp25.encrypt_batch(teng, c.mpk, tm, ti, ta, tb, tp, label_of, **kw)
        assert same_on_tensors(got[0], c.C1) and same_on_tensors(got[1], c.C2), kw


def test_encrypt_seeded_empty_and_refusals(oracle, eng, b4):
    del eng.draws[:]
    rng = Randomness(eng, SEED)
    seeded = afp25.encrypt_batch_seeded(eng, b4.mpk, b4.messages, b4.ids, rng, b4.points, b4.label_of)
    assert eng.draws == [(b4.n, 0, 0), (b4.n, 1, 0)] and rng.next_stream == 2
    again = Randomness(eng, SEED)
    r1 = again.scalars(b4.messages, b4.n)
    want = afp25.encrypt_batch(eng, b4.mpk, b4.messages, b4.ids, r1, again.scalars(b4.messages, b4.n), b4.points, b4.label_of)
    assert same(seeded[0], want[0]) and same(seeded[1], want[1])
    # nothing to do: no engine call and no draw
    none = np.zeros((0, 384), np.uint8)
    empty = afp25.encrypt_batch(Untouchable(), b4.mpk, none, [], [], [], b4.points, np.zeros(0, np.int64))
    assert empty[0].shape == (0, 3, 128) and empty[1].shape == (0, 384)
    rng = Randomness(Untouchable(), SEED)
    assert afp25.encrypt_batch_seeded(Untouchable(), b4.mpk, none, [], rng, b4.points[:1])[1].shape == (0, 384) and rng.next_stream == 0
    # every refusal before the first engine call
    off = Untouchable()
    enc = lambda **kw: afp25.encrypt_batch(off, b4.mpk, kw.pop("messages", b4.messages), kw.pop("ids", b4.ids), b4.r1, b4.r2, kw.pop("points", b4.points),
                                           kw.pop("label_of", b4.label_of), **kw)
    outside, negative = b4.label_of.copy(), b4.label_of.copy()
    outside[3], negative[0] = 3, -1
    tables, gt_two = afp25.encrypt_tables(eng, b4.mpk), eng.GTFixedBase(np.tile(b4.messages[:1], (2, 1)))
    two_bases = afp25.srs_table(eng, G1, b4.mpk["G1ExpTauPowers"][:1])
    for bad in (lambda: enc(label_of=outside), lambda: enc(label_of=negative), lambda: enc(label_of=None), lambda: enc(label_of=b4.label_of[:-1]),
                lambda: enc(label_of=b4.label_of.astype(np.float64)), lambda: enc(route="auto"), lambda: enc(messages=b4.messages.reshape(-1)[:-1]),
                lambda: enc(points=b4.points.reshape(-1)[:-1]), lambda: enc(ids=b4.ids[:-1]), lambda: enc(gt_table=gt_two), lambda: enc(tables=two_bases),
                lambda: enc(route="items", gt_table=gt_two), lambda: enc(bases=b4.messages[:2]), lambda: enc(messages=tensors(b4.messages)[0])):
        with pytest.raises(ValueError):
            bad()
    assert tables.calls == 0


@pytest.mark.parametrize("name", ["b4", "b65", "b1"])
def test_compute_key_and_the_round_trip(oracle, eng, name):
    c = cases.case(oracle, name)
    mpk = afp25.keygen(eng, c.B, c.tau, c.msk)
    table = afp25.srs_table(eng, G1, mpk["G1ExpTauPowers"])
    points = afp25.label_points(eng, c.labels)
    C1, C2 = afp25.encrypt_batch(eng, mpk, c.messages, c.ids, c.r1, c.r2, points, c.label_of if c.k > 1 else None, tables=afp25.encrypt_tables(eng, mpk), route="items")
    D = afp25.digests_ragged(eng, table, c.ids, c.counts)
    assert same(D, c.D)
    sk = afp25.compute_key_batch(eng, c.msk, D, points)
    assert sk.shape == (c.k, 64) and same(sk, c.sk)
    m, ok = afp25.decrypt_batches_ragged(eng, table, c.ids, c.counts, sk, C1, C2, D)
    assert ok.tolist() == [1] * c.n and same(m, c.messages)                    # every message comes back
    td, tp, tmsk, tids, tsk, tc1, tc2 = tensors(D, points, kbytes([c.msk]), kbytes(c.ids), sk, C1, C2)
    assert same_on_tensors(afp25.compute_key_batch(TensorEngine(eng), tmsk, td, tp), c.sk)
    tm, tok = afp25.decrypt_batches_ragged(TensorEngine(eng), table, tids, c.counts, tsk, tc1, tc2, td)
    assert same_on_tensors(tm, c.messages) and tok.tolist() == [1] * c.n
    if name != "b4":
        return
    # one point for all, and nothing to do
    one = afp25.compute_key_batch(eng, c.msk, D, points[1])
    assert same(one[1], c.sk[1]) and not same(one[0], c.sk[0])
    assert afp25.compute_key_batch(Untouchable(), c.msk, np.zeros((0, 64), np.uint8), points[:1]).shape == (0, 64)
    for bad in (lambda: afp25.compute_key_batch(Untouchable(), c.msk, D, points[:2]), lambda: afp25.compute_key_batch(Untouchable(), [1, 2], D, points),
                lambda: afp25.compute_key_batch(Untouchable(), c.msk, D.reshape(-1)[:-1], points), lambda: afp25.compute_key_batch(Untouchable(), c.msk, D, points.tolist()),
                lambda: afp25.compute_key_batch(Untouchable(), c.msk, D.tolist(), points), lambda: afp25.label_bases(Untouchable(), c.mpk, points.tolist())):
        with pytest.raises(ValueError):
            bad()
    # a ciphertext made under another label than its key's decrypts to a different message
    swapped = np.array([0, 2, 2, 2, 1, 1, 1, 1])
    X1, X2 = afp25.encrypt_batch(eng, mpk, c.messages, c.ids, c.r1, c.r2, points, swapped)
    wrong, wok = afp25.decrypt_batches_ragged(eng, table, c.ids, c.counts, sk, X1, X2, D)
    assert wok.tolist() == [1] * c.n and same(wrong[0], c.messages[0]) and same(wrong[6], c.messages[6])      # item 6 has r2 = 0: no label in it
    assert all(not same(wrong[i], c.messages[i]) for i in (1, 2, 3, 4, 5, 7))
    # An identity outside its batch: ok = 0 and a zero row, the neighbours' proofs unchanged.  decrypt_batches_ragged makes the batch
    # polynomial from the very identities it is given, so an outsider cannot be put to it: handed in, it IS a member of the batch.  The
    # stage that decides the rule, table.openings, takes the polynomial apart from the identities (coeffs=), so the outsider goes there,
    # against the true batch's polynomial; through decrypt_batches_ragged the rule shows with a duplicated identity, below.
    ids = list(c.ids)
    ids[5] = cases.sc("outsider")
    f = eng.fr_poly_from_roots_segments(c.ids, c.counts, table.nbase)
    pi, pok = table.openings(kbytes(ids), c.counts, coeffs=f.reshape(-1))
    mine, _ = table.openings(kbytes(c.ids), c.counts, coeffs=f.reshape(-1))
    assert pok.tolist() == [1, 1, 1, 1, 1, 0, 1, 1] and not pi[5].any() and mine[5].any() and same(np.delete(pi, 5, 0), np.delete(mine, 5, 0))
    dup = list(c.ids)
    dup[5] = dup[4]                                                            # ... and one that comes twice in the batch list
    m2, ok2 = afp25.decrypt_batches_ragged(eng, table, dup, c.counts, sk, C1, C2, D)
    assert ok2.tolist() == [1, 1, 1, 1, 0, 0, 1, 1] and not m2[4].any() and not m2[5].any() and same(m2[:4], c.messages[:4])
