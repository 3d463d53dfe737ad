"""The GWWW25 batched-IBE planner (gopairingbasedcryptography_amd/gwww25.py) and the ragged AFP25 planners (afp25.opening_proofs_fused,
decrypt_batches_ragged) over the stand-in engine of tests/standin_openings.py, without a GPU.  Every key and ciphertext component is held
against the line-by-line transcription of bibe/gwww25_bibe/gwww25_bibe.go (:82-256) and gwww25_bibe_utils.go (:9-50) in
tests/gwww25_reference.py, oracle calls and Python integers modulo r: B = 4 with batches of 4, 2 and 1 identities; decrypt(encrypt(M)) == M; a key for another label or
another digest gives another element; an identity outside the batch and a duplicated one give ok = 0 and a zero message where the reference
returns its error; the tables path of Encrypt gives the same bytes and makes no g1_scalar_mul / gt_exp; the tensor path gives the same
bytes; the seeded forms draw in the documented order."""
import numpy as np
import pytest

import bn254_py as o
from standin_engine import TensorEngine, recorded, same_on_tensors, tensors
from standin_openings import OpeningsStandIn
from gwww25_reference import G1, G2, Ref, row, sc
from sw05_fixture import kbytes, kints
from gopairingbasedcryptography_amd import afp25, gwww25
from gopairingbasedcryptography_amd.rng import Randomness

R = o.R
SEED = bytes(range(32))
B = 4
COUNTS = [4, 2, 1]


class Case:
    """three batches of 4, 2 and 1 identities under B = 4, a label per batch, every identity with a message of its own"""

    def __init__(self, orc):
        self.ref = Ref(orc, B)
        self.n = sum(COUNTS)
        self.ids = [sc("id", i) for i in range(self.n)]
        self.of_item = [j for j, c in enumerate(COUNTS) for _ in range(c)]
        self.tg = [sc("tg", j) for j in range(len(COUNTS))]
        self.s = [sc("s", i) for i in range(self.n)]
        self.r, self.y = ([sc(name, j) for j in range(len(COUNTS))] for name in ("r", "y"))
        e = orc.pair_batch(G1, G2)[0]
        self.messages = np.asarray(orc.gt_exp(np.tile(e, (self.n, 1)), kbytes([sc("msg", i) for i in range(self.n)]))).reshape(self.n, 384)
        self.batches = [self.ids[sum(COUNTS[:j]):sum(COUNTS[:j + 1])] for j in range(len(COUNTS))]
        self.ct = [self.ref.encrypt(self.messages[i], self.ids[i], self.tg[self.of_item[i]], self.s[i]) for i in range(self.n)]
        self.D = [self.ref.digest(b) for b in self.batches]
        self.sk = [self.ref.compute_key(self.D[j], self.tg[j], self.r[j], self.y[j]) for j in range(len(COUNTS))]

    def ct_arrays(self):
        return tuple(np.stack([c[t] for c in self.ct]) for t in range(4))


@pytest.fixture(scope="module")
def eng(oracle):
    return OpeningsStandIn(oracle)


@pytest.fixture(scope="module")
def case(oracle):
    return Case(oracle)


@pytest.fixture(scope="module")
def mpk(eng, case):
    r = case.ref
    return gwww25.keygen(eng, B, r.tau, r.w, r.v, r.h, r.alpha)


def test_keygen_is_the_reference(eng, case, mpk):
    r = case.ref
    assert sorted(mpk) == sorted(["G2ExpTauPowers", "G1ExpTau", "G1ExpW", "G1ExpWTau", "G1ExpV", "G1ExpH", "GTExpAlpha"])
    assert mpk["G2ExpTauPowers"].shape == (B, 128) and mpk["G2ExpTauPowers"].tobytes() == np.stack(r.powers).tobytes()
    for name, want in (("G1ExpTau", r.g1_tau), ("G1ExpW", r.g1_w), ("G1ExpWTau", r.g1_wtau), ("G1ExpV", r.g1_v), ("G1ExpH", r.g1_h), ("GTExpAlpha", r.gt_alpha)):
        assert mpk[name].tobytes() == want.tobytes(), name
    for bad in (0, 1025, True, 2.0):
        with pytest.raises(ValueError, match="invalid B"):
            gwww25.keygen(eng, bad, 1, 2, 3, 4, 5)
    # seeded: ONE draw of five scalars in the order tau, w, v, h, alpha
    del eng.draws[:]
    rng = Randomness(eng, SEED)
    mpk2, msk2 = gwww25.keygen_seeded(eng, 2, rng)
    assert eng.draws == [(5, 0, 0)] and rng.next_stream == 1
    tau, w, v, h, alpha = kints(Randomness(eng, SEED).scalars(np.zeros(0, np.uint8), 5))
    assert msk2 == (w, v, h, alpha)
    again = gwww25.keygen(eng, 2, tau, w, v, h, alpha)
    assert all(mpk2[k].tobytes() == again[k].tobytes() for k in again) and mpk2["G2ExpTauPowers"].shape == (2, 128)


def test_encrypt_is_the_reference_with_and_without_tables(eng, case, mpk):
    tg_items = [case.tg[j] for j in case.of_item]
    want = case.ct_arrays()
    calls = recorded(eng, ["g1_scalar_mul_base", "g1_scalar_mul", "g1_sub", "g1_add", "gt_exp", "gt_mul", "fr_mul"])
    got = gwww25.encrypt_batch(eng, mpk, case.messages, case.ids, tg_items, case.s)
    assert [x.shape for x in got] == [(case.n, 64), (case.n, 64), (case.n, 64), (case.n, 384)]
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    assert [name for name, _ in calls] == ["g1_scalar_mul_base", "fr_mul", "g1_scalar_mul", "g1_scalar_mul", "g1_sub", "g1_scalar_mul", "g1_add", "g1_scalar_mul", "gt_exp", "gt_mul"]
    # one label for all: the items of batch 0 alone
    first = gwww25.encrypt_batch(eng, mpk, case.messages[:4], case.ids[:4], case.tg[0], case.s[:4])
    assert all(g.tobytes() == w[:4].tobytes() for g, w in zip(first, want))
    # the tables path: the same bytes, and no g1_scalar_mul / gt_exp
    tables = gwww25.encrypt_tables(eng, mpk)
    assert tables[0].nbase == 4 and tables[1].nbase == 1 and tables[0].bases[1].tobytes() == eng.g1_neg(mpk["G1ExpW"]).tobytes()
    del calls[:]
    fast = gwww25.encrypt_batch(eng, mpk, case.messages, case.ids, tg_items, case.s, tables=tables)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(fast, want))
    assert not {"g1_scalar_mul", "gt_exp"} & {name for name, _ in calls} and tables[0].calls == 2 and tables[1].calls == [(case.n, 1, 1)]
    # the tensor path: CPU tensors through the same planner
    teng = TensorEngine(eng)
    tm, ti, tt, ts = tensors(case.messages, kbytes(case.ids), kbytes(tg_items), kbytes(case.s))
    for tb in (None, tables):
        assert all(same_on_tensors(g, w) for g, w in zip(gwww25.encrypt_batch(teng, mpk, tm, ti, tt, ts, tables=tb), want))
    # seeded: one draw, s
    del eng.draws[:]
    rng = Randomness(eng, SEED)
    seeded = gwww25.encrypt_batch_seeded(eng, mpk, case.messages, case.ids, tg_items, rng)
    assert eng.draws == [(case.n, 0, 0)] and rng.next_stream == 1
    s = Randomness(eng, SEED).scalars(case.messages, case.n)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(seeded, gwww25.encrypt_batch(eng, mpk, case.messages, case.ids, tg_items, s)))
    # nothing to do, and malformed arguments
    assert [x.shape for x in gwww25.encrypt_batch(eng, mpk, np.zeros((0, 384), np.uint8), [], 5, [])] == [(0, 64), (0, 64), (0, 64), (0, 384)]
    for bad in (lambda: gwww25.encrypt_batch(eng, mpk, case.messages, case.ids[:3], 5, case.s), lambda: gwww25.encrypt_batch(eng, mpk, case.messages, case.ids, [1, 2], case.s),
                lambda: gwww25.encrypt_batch(eng, mpk, case.messages.reshape(-1)[:-1], case.ids, 5, case.s),
                lambda: gwww25.encrypt_batch(eng, mpk, case.messages, case.ids, 5, case.s, tables=(tables[0], eng.GTFixedBase(np.tile(mpk["GTExpAlpha"], (2, 1)))))):
        with pytest.raises(ValueError):
            bad()


def test_digests_and_keys_are_the_reference(eng, case, mpk):
    table = gwww25.srs_table(eng, mpk)
    assert table.g2 and table.nbase == B + 1 and table.bases[0].tobytes() == G2.tobytes() and table.bases[1:].tobytes() == mpk["G2ExpTauPowers"].tobytes()
    D = gwww25.digests(eng, table, case.ids, COUNTS)
    assert D.shape == (len(COUNTS), 128) and D.tobytes() == np.stack(case.D).tobytes()
    with pytest.raises(ValueError, match="identities is empty"):
        gwww25.digests(eng, table, case.ids[:4], [4, 0])
    with pytest.raises(ValueError, match="identities is empty"):
        gwww25.digests(eng, table, [], [])
    with pytest.raises(ValueError, match="too many identities for batch size"):
        gwww25.digests(eng, table, case.ids[:5], [5])
    with pytest.raises(ValueError, match="identities is empty"):
        case.ref.digest([])
    with pytest.raises(ValueError, match="too many identities"):
        case.ref.digest(case.ids[:5])
    msk = (case.ref.w, case.ref.v, case.ref.h, case.ref.alpha)
    y, u1, u2 = gwww25.compute_key_batch(eng, msk, D, case.tg, case.r, case.y)
    assert y.shape == (3, 32) and u1.shape == (3, 128) and u2.shape == (3, 128) and kints(y) == case.y
    for j, (_, ru1, ru2) in enumerate(case.sk):
        assert u1[j].tobytes() == ru1.tobytes() and u2[j].tobytes() == ru2.tobytes(), j
    # one label for all digests, the tensor path, and the seeded form: two draws, r then y
    one = gwww25.compute_key_batch(eng, msk, D, case.tg[1], case.r, case.y)
    assert one[2][1].tobytes() == u2[1].tobytes() and one[2][0].tobytes() != u2[0].tobytes() and one[1].tobytes() == u1.tobytes()
    td, tt, tr, ty = tensors(D, kbytes(case.tg), kbytes(case.r), kbytes(case.y))
    assert all(same_on_tensors(g, w) for g, w in zip(gwww25.compute_key_batch(TensorEngine(eng), msk, td, tt, tr, ty), (y, u1, u2)))
    del eng.draws[:]
    rng = Randomness(eng, SEED)
    seeded = gwww25.compute_key_batch_seeded(eng, msk, D, case.tg, rng)
    assert eng.draws == [(3, 0, 0), (3, 1, 0)] and rng.next_stream == 2
    again = Randomness(eng, SEED)
    r = again.scalars(D, 3)
    want = gwww25.compute_key_batch(eng, msk, D, case.tg, r, again.scalars(D, 3))
    assert all(g.tobytes() == w.tobytes() for g, w in zip(seeded, want))
    assert [x.shape for x in gwww25.compute_key_batch(eng, msk, np.zeros((0, 128), np.uint8), 5, [], [])] == [(0, 32), (0, 128), (0, 128)]


def test_decrypt_is_the_reference(eng, case, mpk):
    table = gwww25.srs_table(eng, mpk)
    ct = case.ct_arrays()
    sk = tuple(np.stack([row(kbytes([k[0]])) if t == 0 else k[t] for k in case.sk]) for t in range(3))
    m, ok = gwww25.decrypt_batches(eng, table, case.ids, COUNTS, sk, ct)
    assert m.shape == (case.n, 384) and ok.tolist() == [1] * case.n and m.tobytes() == case.messages.tobytes()          # decrypt(encrypt(M)) == M
    assert table.openings_calls == [tuple(COUNTS)]
    for i in (0, 3, 4, 6):
        j = case.of_item[i]
        assert m[i].tobytes() == case.ref.decrypt(case.sk[j], case.batches[j], case.ids[i], case.ct[i]).tobytes(), i
    # a key per item gives the same; a key for another label or another digest gives another element — the reference's, too
    per_item = tuple(x[case.of_item] for x in sk)
    assert gwww25.decrypt_batches(eng, table, case.ids, COUNTS, per_item, ct)[0].tobytes() == m.tobytes()
    other_label = case.ref.compute_key(case.D[0], case.tg[1], case.r[0], case.y[0])
    other_digest = case.ref.compute_key(case.D[1], case.tg[0], case.r[0], case.y[0])
    for key in (other_label, other_digest):
        rows = tuple(np.stack([row(kbytes([key[0]])) if t == 0 else key[t]]) for t in range(3))
        wrong, wok = gwww25.decrypt_batches(eng, table, case.ids[:4], [4], rows, tuple(x[:4] for x in ct))
        assert wok.tolist() == [1] * 4 and all(wrong[i].tobytes() != case.messages[i].tobytes() for i in range(4))
        assert wrong[2].tobytes() == case.ref.decrypt(key, case.batches[0], case.ids[2], case.ct[2]).tobytes()
    # an identity outside the batch and a duplicated one: ok = 0 and zero rows here, the error there; the neighbours decrypt
    batch0_sk, ct0 = tuple(x[:1] for x in sk), tuple(x[:4] for x in ct)
    outsider = sc("outsider")                                                  # decrypting for an identity the batch does not hold,
    f0 = eng.fr_poly_from_roots_segments(case.batches[0], [4], table.nbase)    # against the batch's own polynomial
    m2, ok2 = gwww25.decrypt_batches(eng, table, [case.ids[0], outsider, case.ids[2], case.ids[3]], [4], batch0_sk, ct0, coeffs=f0)
    assert ok2.tolist() == [1, 0, 1, 1] and not m2[1].any() and m2[[0, 2, 3]].tobytes() == case.messages[[0, 2, 3]].tobytes()
    with pytest.raises(ValueError, match="identity not found"):
        case.ref.decrypt(case.sk[0], case.batches[0], outsider, case.ct[1])
    dup = [case.ids[0], case.ids[1], case.ids[0], case.ids[3]]                 # a batch list with identity 0 twice
    m3, ok3 = gwww25.decrypt_batches(eng, table, dup, [4], batch0_sk, ct0)
    assert ok3.tolist() == [0, 1, 0, 1] and not m3[0].any() and not m3[2].any() and m3[1].any() and m3[3].any()
    with pytest.raises(ValueError, match="identity not found"):
        case.ref.decrypt(case.sk[0], dup, case.ids[0], case.ct[0])
    assert m3[1].tobytes() == case.ref.decrypt(case.sk[0], dup, case.ids[1], case.ct[1]).tobytes()
    # the tensor path
    teng = TensorEngine(eng)
    tids, = tensors(kbytes(case.ids))
    tm, tok = gwww25.decrypt_batches(teng, table, tids, COUNTS, tuple(tensors(*sk)), tuple(tensors(*ct)))
    assert same_on_tensors(tm, m) and same_on_tensors(tok, ok)
    # malformed arguments
    for bad in (lambda: gwww25.decrypt_batches(eng, table, case.ids, [4, 3], sk, ct), lambda: gwww25.decrypt_batches(eng, table, case.ids, [4, 2, 0, 1], sk, ct),
                lambda: gwww25.decrypt_batches(eng, table, case.ids, COUNTS, tuple(x[:2] for x in sk), ct),
                lambda: gwww25.decrypt_batches(eng, table, case.ids, COUNTS, sk, tuple(x[:5] for x in ct))):
        with pytest.raises(ValueError):
            bad()


def test_afp25_fused_openings_equal_the_chunked_route(eng, oracle):
    """full batches: opening_proofs_fused is opening_proofs byte for byte; ragged batches decrypt as the per-batch host statement does"""
    tau, Bq = sc("afp-tau"), 3
    tau_powers = np.asarray(oracle.g1_scalar_mul(G1, kbytes([pow(tau, i, R) for i in range(1, Bq + 1)]))).reshape(Bq, 64)
    table = afp25.srs_table(eng, G1, tau_powers)
    ids = [[sc("afp-id", 3 * j + i) for i in range(Bq)] for j in range(2)]
    old = afp25.opening_proofs(eng, table, ids)
    pi, ok = afp25.opening_proofs_fused(eng, table, ids)
    assert ok.tolist() == [1] * 6 and pi.tobytes() == np.asarray(old).tobytes()
    flat = [x for r in ids for x in r]
    ragged, rok = afp25.opening_proofs_fused(eng, table, flat[:5], [3, 2])
    assert rok.tolist() == [1] * 5 and ragged[:3].tobytes() == pi[:3].tobytes() and ragged[3:].tobytes() != pi[3:5].tobytes()
    D = afp25.digests_ragged(eng, table, flat[:5], [3, 2])
    for j, batch in enumerate((flat[:3], flat[3:5])):
        assert D[j].tobytes() == np.asarray(afp25.digest(eng, G1, tau_powers, batch)[0]).reshape(64).tobytes()
    # decryption of ragged batches against the per-item host statement (decrypt_batch), on made-up ciphertexts: the same GT bytes
    sk = np.asarray(oracle.g1_scalar_mul(G1, kbytes([sc("afp-sk", j) for j in range(2)]))).reshape(2, 64)
    C1 = np.asarray(oracle.g2_scalar_mul(G2, kbytes([sc("afp-c1", i) for i in range(15)]))).reshape(5, 3, 128)
    e = oracle.pair_batch(G1, G2)[0]
    C2 = np.asarray(oracle.gt_exp(np.tile(e, (5, 1)), kbytes([sc("afp-c2", i) for i in range(5)]))).reshape(5, 384)
    m, mok = afp25.decrypt_batches_ragged(eng, table, flat[:5], [3, 2], sk, C1, C2)
    assert mok.tolist() == [1] * 5
    a = 0
    for j, batch in enumerate((flat[:3], flat[3:5])):
        Dj, f = afp25.digest(eng, G1, tau_powers, batch)
        want = afp25.decrypt_batch(eng, G1, tau_powers, Dj, f, sk[j], [(batch[i], C1[a + i], C2[a + i]) for i in range(len(batch))], identities=batch)
        assert m[a:a + len(batch)].tobytes() == np.asarray(want).tobytes(), j
        a += len(batch)
    dup, dok = afp25.decrypt_batches_ragged(eng, table, [flat[0], flat[1], flat[0], flat[3], flat[4]], [3, 2], sk, C1, C2)
    assert dok.tolist() == [0, 1, 0, 1, 1] and not dup[0].any() and not dup[2].any() and dup[3:].tobytes() == m[3:].tobytes()
    for bad, text in ((lambda: afp25.opening_proofs_fused(eng, table, flat[:4], [4]), "too many"), (lambda: afp25.opening_proofs_fused(eng, table, flat[:3], [3, 0]), "empty"),
                      (lambda: afp25.opening_proofs_fused(eng, table, flat[:5]), "whole number")):
        with pytest.raises(ValueError, match=text):
            bad()
