"""AFP25 KeyGen / Encrypt / ComputeKey on the MI355X (run with -m gpu) through gopairingbasedcryptography_amd/afp25.py on the GPU engine:
the cases and the expectations of tests/afp25_scheme_cases.py (the scheme's equations in scalars through the CPU oracle) on CUDA tensors,
and on host arrays for the B = 4 case; every pair of routes the same bytes; the seeded forms against the plain forms on the scalars of a
second Randomness; and the round trip keygen -> srs_table -> encrypt_batch -> digests_ragged -> compute_key_batch ->
decrypt_batches_ragged back to the messages.  At most 65 x 3 pairs per test."""
import numpy as np
import pytest

import afp25_scheme_cases as cases
from afp25_scheme_cases import G1, R
from sw05_fixture import kbytes, kints
from gopairingbasedcryptography_amd import afp25
from gopairingbasedcryptography_amd.rng import Randomness

pytestmark = pytest.mark.gpu
SEED = bytes((29 * i + 3) % 256 for i in range(32))
NAMES = ["b4", "b65", "b1"]


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def dev(*arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda() for a in arrays]
    return out[0] if len(out) == 1 else out


def back(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def same(got, want):
    return tuple(got.shape) == np.asarray(want).shape and back(got).tobytes() == np.asarray(want).tobytes()


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 64, 65, 1024])
def test_tau_powers_on_the_device(eng, B):
    tau = cases.sc("powers-tau") + R
    got = afp25.tau_powers(eng, dev(np.frombuffer(tau.to_bytes(32, "little"), dtype=np.uint8)), B)
    assert got.is_cuda and tuple(got.shape) == (B, 32) and kints(back(got)) == [pow(tau, i, R) for i in range(1, B + 1)]


@pytest.mark.parametrize("name", NAMES)
def test_keygen_is_the_equations(oracle, eng, name):
    c = cases.case(oracle, name)
    mpk = afp25.keygen(eng, c.B, *dev(kbytes([c.tau]), kbytes([c.msk])))
    assert sorted(mpk) == ["G1ExpTauPowers", "G2ExpMsk", "G2ExpTau"] and all(isinstance(v, np.ndarray) and same(v, c.mpk[k]) for k, v in mpk.items())
    if name == "b4":
        host = afp25.keygen(eng, c.B, c.tau, c.msk)
        assert all(same(v, c.mpk[k]) for k, v in host.items())


def test_keygen_seeded_keeps_the_draw_order(eng):
    import torch
    like = torch.zeros(0, dtype=torch.uint8, device="cuda")
    rng = Randomness(eng, SEED)
    mpk, msk = afp25.keygen_seeded(eng, 5, rng, like=like)
    assert rng.next_stream == 1 and msk.is_cuda and tuple(msk.shape) == (32,)
    want_msk, want_tau = kints(Randomness(eng, SEED).scalars(np.zeros(0, np.uint8), 2))
    assert kints(back(msk)) == [want_msk]
    again = afp25.keygen(eng, 5, want_tau, want_msk)
    assert all(same(mpk[k], again[k]) for k in again)
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="invalid B"):
            afp25.keygen_seeded(eng, bad, rng, like=like)
    assert rng.next_stream == 1


@pytest.mark.parametrize("name", NAMES)
def test_encrypt_is_the_equations_on_every_route(oracle, eng, name):
    import torch
    c = cases.case(oracle, name)
    label_of = c.label_of if c.k > 1 else None
    data = dev(np.frombuffer(b"".join(c.labels) or b"\0", dtype=np.uint8))
    off = torch.from_numpy(np.cumsum([0] + [len(t) for t in c.labels]).astype(np.int64)).cuda()
    points = afp25.label_points(eng, data, off)
    assert points.is_cuda and same(points, c.points) and same(afp25.label_points(eng, c.labels), c.points)
    bases = afp25.label_bases(eng, c.mpk, points)
    args = dev(c.messages, kbytes(c.ids), kbytes(c.r1), kbytes(c.r2))
    tables, gt_table = afp25.encrypt_tables(eng, c.mpk), eng.GTFixedBase(bases)
    try:
        for kw in (dict(), dict(bases=bases), dict(tables=tables), dict(gt_table=gt_table), dict(tables=tables, gt_table=gt_table), dict(route="items"),
                   dict(tables=tables, route="items")):
            C1, C2 = afp25.encrypt_batch(eng, c.mpk, *args, points, label_of, **kw)
            assert C1.is_cuda and C2.is_cuda and same(C1, c.C1) and same(C2, c.C2), kw
        if name == "b4":                                                       # host arrays and Python integers, every route
            assert not c.C1[2, 1].any() and not c.C1[6, 2].any() and same(c.C2[6], c.messages[6])
            hbases = back(bases)
            for kw in (dict(), dict(tables=tables, bases=hbases), dict(gt_table=gt_table), dict(tables=tables, route="items")):
                C1, C2 = afp25.encrypt_batch(eng, c.mpk, c.messages, c.ids, c.r1, c.r2, c.points, label_of, **kw)
                assert isinstance(C1, np.ndarray) and same(C1, c.C1) and same(C2, c.C2), kw
            rng = Randomness(eng, SEED)
            seeded = afp25.encrypt_batch_seeded(eng, c.mpk, args[0], args[1], rng, points, label_of, tables=tables)
            again = Randomness(eng, SEED)
            r1 = again.scalars(args[0], c.n)
            want = afp25.encrypt_batch(eng, c.mpk, args[0], args[1], r1, again.scalars(args[0], c.n), points, label_of)
            assert rng.next_stream == 2 and torch.equal(seeded[0], want[0]) and torch.equal(seeded[1], want[1])
            empty = afp25.encrypt_batch(eng, c.mpk, args[0][:0], args[1][:0], args[2][:0], args[3][:0], points, label_of[:0], tables=tables)
            assert tuple(empty[0].shape) == (0, 3, 128) and tuple(empty[1].shape) == (0, 384) and empty[1].is_cuda
            outside = label_of.copy()
            outside[2] = 3
            with pytest.raises(ValueError, match="label_of"):
                afp25.encrypt_batch(eng, c.mpk, *args, points, outside)
    finally:
        tables.close(), gt_table.close()


@pytest.mark.parametrize("name", NAMES)
def test_compute_key_and_the_round_trip(oracle, eng, name):
    c = cases.case(oracle, name)
    label_of = c.label_of if c.k > 1 else None
    tau, msk, messages, ids, r1, r2 = dev(kbytes([c.tau]), kbytes([c.msk]), c.messages, kbytes(c.ids), kbytes(c.r1), kbytes(c.r2))
    mpk = afp25.keygen(eng, c.B, tau, msk)
    table, tables = afp25.srs_table(eng, G1, mpk["G1ExpTauPowers"]), afp25.encrypt_tables(eng, mpk)
    try:
        points = afp25.label_points(eng, c.labels)
        C1, C2 = afp25.encrypt_batch(eng, mpk, messages, ids, r1, r2, dev(points), label_of, tables=tables)
        D = afp25.digests_ragged(eng, table, ids, c.counts)
        assert same(D, c.D)
        sk = afp25.compute_key_batch(eng, msk, D, dev(points))
        assert sk.is_cuda and same(sk, c.sk)
        m, ok = afp25.decrypt_batches_ragged(eng, table, ids, c.counts, sk, C1, C2, D)
        assert back(ok).tolist() == [1] * c.n and same(m, c.messages)          # every message comes back
        if name != "b4":
            return
        hsk = afp25.compute_key_batch(eng, c.msk, back(D), points)              # host arrays
        assert isinstance(hsk, np.ndarray) and same(hsk, c.sk)
        hm, hok = afp25.decrypt_batches_ragged(eng, table, c.ids, c.counts, hsk, back(C1), back(C2), back(D))
        assert hok.tolist() == [1] * c.n and same(hm, c.messages)
        one = afp25.compute_key_batch(eng, msk, D, points[1])                  # one point for all, given on the host
        assert same(one[1], c.sk[1]) and not same(one[0], c.sk[0])
        # another label than the key's: another message (item 6 has r2 = 0 and carries no label)
        swapped = np.array([0, 2, 2, 2, 1, 1, 1, 1])
        X1, X2 = afp25.encrypt_batch(eng, mpk, messages, ids, r1, r2, dev(points), swapped, route="items")
        wrong, wok = afp25.decrypt_batches_ragged(eng, table, ids, c.counts, sk, X1, X2, D)
        wrong = back(wrong)
        assert back(wok).tolist() == [1] * c.n and same(wrong[0], c.messages[0]) and same(wrong[6], c.messages[6])
        assert all(not same(wrong[i], c.messages[i]) for i in (1, 2, 3, 4, 5, 7))
        # An identity outside its batch: ok = 0 and a zero row, the neighbours' proofs unchanged.  decrypt_batches_ragged makes the batch
        # polynomial from the identities it is given, so the outsider goes to the stage that decides the rule, table.openings, against
        # the true batch's polynomial (coeffs=).
        out_ids = list(c.ids)
        out_ids[5] = cases.sc("outsider")
        f = eng.fr_poly_from_roots_segments(ids.reshape(-1), c.counts, table.nbase)
        pi, pok = table.openings(dev(kbytes(out_ids)).reshape(-1), c.counts, coeffs=f.reshape(-1))
        mine, mok = table.openings(ids.reshape(-1), c.counts, coeffs=f.reshape(-1))
        pi, mine = back(pi), back(mine)
        assert back(pok).tolist() == [1, 1, 1, 1, 1, 0, 1, 1] and back(mok).tolist() == [1] * c.n and not pi[5].any() and mine[5].any()
        assert same(np.delete(pi, 5, 0), np.delete(mine, 5, 0))
        # an identity that comes twice in its batch list: ok = 0 and zero rows, the other batches decrypt
        dup = list(c.ids)
        dup[5] = dup[4]
        m2, ok2 = afp25.decrypt_batches_ragged(eng, table, dev(kbytes(dup)), c.counts, sk, C1, C2, D)
        m2 = back(m2)
        assert back(ok2).tolist() == [1, 1, 1, 1, 0, 0, 1, 1] and not m2[4].any() and not m2[5].any() and same(m2[:4], c.messages[:4])
    finally:
        table.close(), tables.close()
