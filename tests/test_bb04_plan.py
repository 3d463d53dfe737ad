"""The Boneh-Boyen IBE planners (gopairingbasedcryptography_amd/bb04sibe.py, bb04ibe.py) and the gt_table option of waters05.py and
gentry06.py over the stand-in engine of tests/standin_gtfixed.py, without a GPU.  Every key and ciphertext component is held against a
straight transcription of the reference's operations in the reference's order (ibe/bb04_sibe/bb04_sibe.go:109-231,
ibe/bb04_ibe/bb04_ibe.go:94-271), written out here with oracle calls and Python integers modulo r: decrypt(encrypt(M)) == M, a key of
another identity gives another element, the sIBE key for ID + x + r y = 0 is the point at infinity, the one-key and the key-per-ciphertext
forms agree, the tensor path gives the same bytes, the seeded forms draw what they document.  BB04 IBE runs at identity length 8 here (and
its key generation also at 20: two groups of 16 terms, the second padded); the GPU test runs the reference's 256.
waters05 / gentry06: with gt_table=None the recorded calls are the ones of a call without the keyword; with a table no gt_exp is left
in Encrypt and every byte is the same."""
import hashlib

import numpy as np
import pytest

import bn254_py as o
from standin_engine import TensorEngine, recorded, same_on_tensors, tensors
from standin_gtfixed import GTFixedStandIn
from sw05_fixture import kbytes, kints
from gopairingbasedcryptography_amd import bb04ibe, bb04sibe, gentry06, waters05
from gopairingbasedcryptography_amd.rng import Randomness

R = o.R
G1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
G2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
SEED = bytes(range(32))


def sc(tag, i=0):
    return o.bench_scalar("bb04-" + tag, i)


def row(x):
    return np.asarray(x, dtype=np.uint8).reshape(-1)


@pytest.fixture(scope="module")
def eng(oracle):
    return GTFixedStandIn(oracle)


# ------------------------------------------------------------------------------------------------ BB04 sIBE
class Sibe:
    """bb04_sibe.go on the oracle, one identity at a time, every line the reference's; identity 2 has ID + x + r y = 0"""
    N = 4

    def __init__(self, orc):
        self.orc = orc
        self.x, self.y = sc("x"), sc("y")
        self.r, self.s, self.msg = ([sc(name, i) for i in range(self.N)] for name in ("r", "s", "msg"))
        self.ids = [sc("id", i) for i in range(self.N)]
        self.ids[2] = (-(self.x + self.r[2] * self.y)) % R
        self.e = row(orc.pair_batch(G1, G2))
        self.messages = np.asarray(orc.gt_exp(np.tile(self.e, (self.N, 1)), kbytes(self.msg))).reshape(self.N, 384)
        self.X, self.Y = (row(orc.g1_scalar_mul(G1, kbytes([v]))) for v in (self.x, self.y))                    # SetUp :112-113

    def keygen(self, i):
        d = self.r[i] * self.y % R                                             # denominator.Mul(&r, &instance.y)
        d = (d + self.x) % R                                                   # .Add(denominator, &instance.x)
        d = (d + self.ids[i]) % R                                              # .Add(denominator, &identity.Id)
        d = pow(d, -1, R) if d else 0                                          # .Inverse: 0 -> 0
        return row(self.orc.g2_scalar_mul(G2, kbytes([d])))                    # ScalarMultiplicationBase

    def encrypt(self, i):
        s, orc = self.s[i], self.orc
        a = orc.g1_scalar_mul(G1, kbytes([s * self.ids[i] % R]))[0]            # s_id, ScalarMultiplicationBase
        x_s = orc.g1_scalar_mul(self.X, kbytes([s]))[0]
        a = row(orc.g1_sum(np.stack([a, x_s])))                                # a.Add(a, x_s)
        b = row(orc.g1_scalar_mul(self.Y, kbytes([s])))
        c = orc.pair_batch(G1, G2)[0]                                          # recomputed, as the reference recomputes it
        c = orc.gt_exp(c, kbytes([s]))[0]
        return a, b, row(orc.gt_mul(c, self.messages[i]))

    def decrypt(self, a, b, c, r, k):
        a_br = self.orc.g1_scalar_mul(b, kbytes([r]))[0]                       # B^r
        a_br = self.orc.g1_sum(np.stack([row(a), a_br]))                       # A + B^r
        return row(self.orc.gt_div(c, self.orc.pair_batch(a_br, k)[0]))        # C / e(A B^r, K)


@pytest.fixture(scope="module")
def sibe(oracle):
    return Sibe(oracle)


def test_sibe_is_the_reference(eng, sibe):
    X, Y = bb04sibe.public_params(eng, sibe.x, sibe.y)
    assert X.tobytes() == sibe.X.tobytes() and Y.tobytes() == sibe.Y.tobytes()
    e = bb04sibe.public_pairing(eng)
    assert e.shape == (384,) and e.tobytes() == sibe.e.tobytes()
    k = bb04sibe.keygen_batch(eng, sibe.x, sibe.y, sibe.ids, sibe.r)
    assert k.shape == (sibe.N, 128)
    for i in range(sibe.N):
        assert k[i].tobytes() == sibe.keygen(i).tobytes(), i
    assert not k[2].any() and all(k[i].any() for i in (0, 1, 3))               # ID + x + r y = 0: the point at infinity
    table = eng.GTFixedBase(e)
    a, b, c = bb04sibe.encrypt_batch(eng, (X, Y), table, sibe.messages, sibe.ids, sibe.s)
    assert a.shape == (sibe.N, 64) and b.shape == (sibe.N, 64) and c.shape == (sibe.N, 384) and table.calls == [(sibe.N, 1, 1)]
    for i in range(sibe.N):
        ra, rb, rc = sibe.encrypt(i)
        assert a[i].tobytes() == ra.tobytes() and b[i].tobytes() == rb.tobytes() and c[i].tobytes() == rc.tobytes(), i
    good = [0, 1, 3]
    m = bb04sibe.decrypt_batch(eng, a[good], b[good], c[good], [sibe.r[i] for i in good], k[good])                # a key per ciphertext
    assert m.tobytes() == sibe.messages[good].tobytes()
    for j, i in enumerate(good):
        assert m[j].tobytes() == sibe.decrypt(a[i], b[i], c[i], sibe.r[i], k[i]).tobytes()
    wrong = bb04sibe.decrypt_batch(eng, a[:1], b[:1], c[:1], sibe.r[1], k[1])                                      # the key of another identity
    assert wrong.tobytes() != sibe.messages[:1].tobytes() and wrong.tobytes() == sibe.decrypt(a[0], b[0], c[0], sibe.r[1], k[1]).tobytes()


def test_sibe_one_key_for_all_tensors_seeded_and_errors(eng, sibe):
    X, Y = bb04sibe.public_params(eng, sibe.x, sibe.y)
    table = eng.GTFixedBase(bb04sibe.public_pairing(eng))
    ids = [sibe.ids[1]] * 3
    k = bb04sibe.keygen_batch(eng, sibe.x, sibe.y, [sibe.ids[1]], [sibe.r[1]])
    a, b, c = bb04sibe.encrypt_batch(eng, (X, Y), table, sibe.messages[:3], ids, sibe.s[:3])
    one = bb04sibe.decrypt_batch(eng, a, b, c, sibe.r[1], k[0])                                                    # one key for all ...
    each = bb04sibe.decrypt_batch(eng, a, b, c, kbytes([sibe.r[1]] * 3), np.tile(k[0], (3, 1)))                    # ... and one per ciphertext
    assert one.tobytes() == each.tobytes() == sibe.messages[:3].tobytes()
    # the tensor path: CPU tensors through the same planner
    teng = TensorEngine(eng)
    tm, ti, ts = tensors(sibe.messages[:3], kbytes(ids), kbytes(sibe.s[:3]))
    ta, tb, tc = bb04sibe.encrypt_batch(teng, (X, Y), table, tm, ti, ts)                                          # (the table stand-in takes tensors itself)
    assert same_on_tensors(ta, a) and same_on_tensors(tb, b) and same_on_tensors(tc, c)
    assert same_on_tensors(bb04sibe.decrypt_batch(teng, ta, tb, tc, sibe.r[1], k[0]), sibe.messages[:3])
    assert same_on_tensors(bb04sibe.keygen_batch(teng, sibe.x, sibe.y, ti[:32], tensors(kbytes([sibe.r[1]]))[0]), k)
    # seeded: one draw each, stream ids in order, and exactly the unseeded result on the scalars drawn
    rng = Randomness(eng, SEED)
    del eng.draws[:]
    r, k2 = bb04sibe.keygen_batch_seeded(eng, sibe.x, sibe.y, sibe.ids, rng)
    a2, b2, c2 = bb04sibe.encrypt_batch_seeded(eng, (X, Y), table, sibe.messages, sibe.ids, rng)
    assert eng.draws == [(sibe.N, 0, 0), (sibe.N, 1, 0)] and rng.next_stream == 2
    assert k2.tobytes() == bb04sibe.keygen_batch(eng, sibe.x, sibe.y, sibe.ids, r).tobytes()
    s = Randomness(eng, SEED)
    s.scalars(sibe.messages, sibe.N)
    want = bb04sibe.encrypt_batch(eng, (X, Y), table, sibe.messages, sibe.ids, s.scalars(sibe.messages, sibe.N))
    assert all(x.tobytes() == y.tobytes() for x, y in zip((a2, b2, c2), want))
    assert bb04sibe.decrypt_batch(eng, a2, b2, c2, r, k2).tobytes() == sibe.messages.tobytes()
    # nothing to do, and malformed arguments
    assert bb04sibe.keygen_batch(eng, sibe.x, sibe.y, [], []).shape == (0, 128)
    empty = bb04sibe.encrypt_batch(eng, (X, Y), table, np.zeros((0, 384), np.uint8), [], [])
    assert [x.shape for x in empty] == [(0, 64), (0, 64), (0, 384)]
    assert bb04sibe.decrypt_batch(eng, *empty, sibe.r[0], k[0]).shape == (0, 384)
    for call in (lambda: bb04sibe.public_params(eng, [1, 2], 3),
                 lambda: bb04sibe.keygen_batch(eng, sibe.x, sibe.y, sibe.ids, sibe.r[:-1]),
                 lambda: bb04sibe.encrypt_batch(eng, (X, Y), table, sibe.messages[:2], sibe.ids[:3], sibe.s[:2]),
                 lambda: bb04sibe.encrypt_batch(eng, (X, Y[:32]), table, sibe.messages[:2], sibe.ids[:2], sibe.s[:2]),
                 lambda: bb04sibe.encrypt_batch(eng, (X, Y), table, sibe.messages.reshape(-1)[:-1], sibe.ids, sibe.s),
                 lambda: bb04sibe.decrypt_batch(eng, a, b[:2], c, sibe.r[1], k[0]),
                 lambda: bb04sibe.decrypt_batch(eng, a, b, c, sibe.r[:2], k[0])):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------------------------------------------------------ BB04 IBE
IDS = ["alice@example.com", "bob@example.com", "身份"]


def ref_bits(s):
    """Id[] of NewBB04IBEIdentity, :258-268: byte by byte, bit 7 first"""
    return [(b >> (7 - t)) & 1 for b in hashlib.sha256(s.encode()).digest() for t in range(8)]


class Ibe:
    """bb04_ibe.go on the oracle at identity length L, one identity at a time, every line the reference's"""

    def __init__(self, orc, L):
        self.orc, self.L, n = orc, L, len(IDS)
        tag = "ibe%d-" % L
        self.alpha, self.u_k = sc(tag + "alpha"), [sc(tag + "u", i) for i in range(2 * L)]
        self.g2_alpha, self.g1_alpha = (row(mul(G, kbytes([self.alpha]))) for mul, G in ((orc.g2_scalar_mul, G2), (orc.g1_scalar_mul, G1)))
        self.uij = np.asarray(orc.g2_scalar_mul(G2, kbytes(self.u_k))).reshape(L, 2, 128)       # uij[i][j], the loop order of SetUp
        self.bits = [ref_bits(s)[:L] for s in IDS]
        self.r = [[sc(tag + "r", i * L + j) for j in range(L)] for i in range(n)]
        self.t, self.msg = ([sc(tag + name, i) for i in range(n)] for name in ("t", "msg"))
        e = row(orc.pair_batch(G1, G2))
        self.messages = np.asarray(orc.gt_exp(np.tile(e, (n, 1)), kbytes(self.msg))).reshape(n, 384)

    def keygen(self, i):
        orc = self.orc
        dj = np.stack([orc.g1_scalar_mul(G1, kbytes([self.r[i][j]]))[0] for j in range(self.L)])
        prod = np.zeros(128, dtype=np.uint8)                                    # SetInfinity
        for j in range(self.L):
            u = orc.g2_scalar_mul(self.uij[j][self.bits[i][j]], kbytes([self.r[i][j]]))[0]
            prod = row(orc.g2_sum(np.stack([prod, u])))                         # prod.Add(prod, uIAiR)
        return row(orc.g2_sum(np.stack([self.g2_alpha, prod]))), dj

    def encrypt(self, i):
        orc, t = self.orc, kbytes([self.t[i]])
        e = orc.pair_batch(self.g1_alpha, G2)[0]                                # recomputed, as the reference recomputes it
        a = row(orc.gt_mul(orc.gt_exp(e, t)[0], self.messages[i]))
        b = row(orc.g1_scalar_mul(G1, t))
        return a, b, np.stack([orc.g2_scalar_mul(self.uij[j][self.bits[i][j]], t)[0] for j in range(self.L)])

    def decrypt(self, d0, dj, a, b, c):
        orc = self.orc
        prod = np.frombuffer(o.gt_to_bytes(o.F12_ONE), dtype=np.uint8)          # SetOne
        for j in range(self.L):
            prod = orc.gt_mul(prod, orc.pair_batch(dj[j], c[j])[0])[0]
        m = orc.gt_mul(a, prod)[0]
        return row(orc.gt_div(m, orc.pair_batch(b, d0)[0]))


@pytest.fixture(scope="module")
def ibe(oracle):
    return Ibe(oracle, 8)


def test_identity_bits_and_index_rows(eng):
    bits = bb04ibe.identity_bits(IDS)
    assert bits.shape == (3, 256) and bits.dtype == np.uint8 and bits.tolist() == [ref_bits(s) for s in IDS]
    assert bb04ibe.identity_bits(IDS, 8).tolist() == [ref_bits(s)[:8] for s in IDS] and bb04ibe.identity_bits([b"bob@example.com"]).tolist() == [ref_bits(IDS[1])]
    assert bb04ibe.identity_bits_device(eng, IDS, length=20).tolist() == [ref_bits(s)[:20] for s in IDS]
    flat = np.frombuffer("".join(IDS).encode(), dtype=np.uint8)
    off = np.cumsum([0] + [len(s.encode()) for s in IDS]).astype(np.uint64)
    assert bb04ibe.identity_bits_device(eng, flat, off).tolist() == bits.tolist()
    t = bb04ibe.identity_bits_device(TensorEngine(eng), tensors(flat)[0], off, length=9)
    assert same_on_tensors(t, np.ascontiguousarray(bits[:, :9]))
    idx = bb04ibe.index_rows(bits)
    assert idx.dtype == np.uint32 and idx.tolist() == [[2 * j + b for j, b in enumerate(r)] for r in bits.tolist()]
    tidx = bb04ibe.index_rows(tensors(bits)[0])
    assert str(tidx.dtype) == "torch.int32" and tidx.numpy().tolist() == idx.tolist()
    assert bb04ibe.identity_bits([]).shape == (0, 256)
    for call in (lambda: bb04ibe.identity_bits(["a", ""]), lambda: bb04ibe.identity_bits(["a"], 0), lambda: bb04ibe.identity_bits(["a"], 257),
                 lambda: bb04ibe.identity_bits_device(eng, ["a", b""]), lambda: bb04ibe.index_rows(bits[0])):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("L", [8, 20])
def test_ibe_keygen_is_the_reference(oracle, eng, L):
    """length 8: one group of 16 terms, half of it INDEX_NONE; length 20: two groups, the second padded, summed per identity"""
    ref = Ibe(oracle, L)
    g1a, g2a, uij = bb04ibe.public_params(eng, ref.alpha, ref.u_k)
    assert g1a.tobytes() == ref.g1_alpha.tobytes() and g2a.tobytes() == ref.g2_alpha.tobytes() and uij.tobytes() == ref.uij.tobytes()
    table = bb04ibe.u_table(eng, uij)
    assert table.g2 and table.nbase == 2 * L
    bits = bb04ibe.identity_bits(IDS, L)
    d0, dj = bb04ibe.keygen_batch(eng, table, g2a, bits, ref.r)
    assert d0.shape == (3, 128) and dj.shape == (3, L, 64) and table.calls == 1
    for i in range(3):
        r0, rj = ref.keygen(i)
        assert d0[i].tobytes() == r0.tobytes() and dj[i].tobytes() == rj.tobytes(), i
    rng = Randomness(eng, SEED)
    del eng.draws[:]
    d0s, djs = bb04ibe.keygen_batch_seeded(eng, table, g2a, bits, rng)
    assert eng.draws == [(3 * L, 0, 0)]
    want = bb04ibe.keygen_batch(eng, table, g2a, bits, Randomness(eng, SEED).scalars(bits, 3, L))
    assert d0s.tobytes() == want[0].tobytes() and djs.tobytes() == want[1].tobytes()


def test_ibe_is_the_reference(eng, ibe):
    L = ibe.L
    g1a, g2a, uij = bb04ibe.public_params(eng, ibe.alpha, ibe.u_k)
    e_alpha = bb04ibe.public_pairing(eng, g1a)
    assert e_alpha.tobytes() == row(ibe.orc.pair_batch(ibe.g1_alpha, G2)).tobytes()
    table, gt_table = bb04ibe.u_table(eng, uij), eng.GTFixedBase(e_alpha)
    bits = bb04ibe.identity_bits(IDS, L)
    d0, dj = bb04ibe.keygen_batch(eng, table, g2a, bits, ibe.r)
    a, b, c = bb04ibe.encrypt_batch(eng, table, gt_table, ibe.messages, bits, ibe.t)
    assert a.shape == (3, 384) and b.shape == (3, 64) and c.shape == (3, L, 128) and gt_table.calls == [(3, 1, 1)] and table.calls == 2
    for i in range(3):
        ra, rb, rc = ibe.encrypt(i)
        assert a[i].tobytes() == ra.tobytes() and b[i].tobytes() == rb.tobytes() and c[i].tobytes() == rc.tobytes(), i
    m = bb04ibe.decrypt_batch(eng, (d0, dj), a, b, c)                                                               # a key per ciphertext
    assert m.tobytes() == ibe.messages.tobytes()
    for i in range(3):
        assert m[i].tobytes() == ibe.decrypt(d0[i], dj[i], a[i], b[i], c[i]).tobytes()
    wrong = bb04ibe.decrypt_batch(eng, (d0[1], dj[1]), a[:1], b[:1], c[:1])                                         # the key of another identity
    assert wrong.tobytes() != ibe.messages[:1].tobytes() and wrong[0].tobytes() == ibe.decrypt(d0[1], dj[1], a[0], b[0], c[0]).tobytes()
    # three messages to one identity: one key for all, and one per ciphertext
    same = np.tile(bits[2], (3, 1))
    a1, b1, c1 = bb04ibe.encrypt_batch(eng, table, gt_table, ibe.messages, same, ibe.t)
    one = bb04ibe.decrypt_batch(eng, (d0[2], dj[2]), a1, b1, c1)
    each = bb04ibe.decrypt_batch(eng, (np.tile(d0[2], (3, 1)), np.tile(dj[2], (3, 1, 1))), a1, b1, c1)
    assert one.tobytes() == each.tobytes() == ibe.messages.tobytes()
    # the tensor path
    teng, ttable = TensorEngine(eng), table                                     # (the table stand-ins take tensors themselves)
    tm, tb_, tt = tensors(ibe.messages, bits, kbytes(ibe.t))
    ta, tb, tc = bb04ibe.encrypt_batch(teng, ttable, gt_table, tm, tb_, tt)
    assert same_on_tensors(ta, a) and same_on_tensors(tb, b) and same_on_tensors(tc, c)
    assert same_on_tensors(bb04ibe.decrypt_batch(teng, (d0, dj), ta, tb, tc), ibe.messages)                         # a host key beside tensors
    td0, tdj = bb04ibe.keygen_batch(teng, ttable, g2a, tb_, tensors(kbytes([v for r in ibe.r for v in r]))[0])
    assert same_on_tensors(td0, d0) and same_on_tensors(tdj, dj)
    # seeded Encrypt: one draw, and exactly the unseeded result on the scalars drawn
    del eng.draws[:]
    got = bb04ibe.encrypt_batch_seeded(eng, table, gt_table, ibe.messages, bits, Randomness(eng, SEED))
    assert eng.draws == [(3, 0, 0)]
    want = bb04ibe.encrypt_batch(eng, table, gt_table, ibe.messages, bits, Randomness(eng, SEED).scalars(bits, 3))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
    assert bb04ibe.decrypt_batch(eng, (d0, dj), *got).tobytes() == ibe.messages.tobytes()
    # nothing to do, and malformed arguments
    none = bits[:0]
    assert [x.shape for x in bb04ibe.keygen_batch(eng, table, g2a, none, [])] == [(0, 128), (0, L, 64)]
    empty = bb04ibe.encrypt_batch(eng, table, gt_table, np.zeros((0, 384), np.uint8), none, [])
    assert [x.shape for x in empty] == [(0, 384), (0, 64), (0, L, 128)]
    assert bb04ibe.decrypt_batch(eng, (d0[0], dj[0]), *empty).shape == (0, 384)
    for call in (lambda: bb04ibe.public_params(eng, ibe.alpha, ibe.u_k[:-1]), lambda: bb04ibe.public_params(eng, [1, 2], ibe.u_k),
                 lambda: bb04ibe.u_table(eng, uij[:-1]), lambda: bb04ibe.u_table(eng, uij.reshape(-1)[:-1]),
                 lambda: bb04ibe.keygen_batch(eng, table, g2a, bits[:, :7], ibe.r), lambda: bb04ibe.keygen_batch(eng, table, g2a, bits, ibe.r[:2]),
                 lambda: bb04ibe.encrypt_batch(eng, table, gt_table, ibe.messages[:2], bits, ibe.t),
                 lambda: bb04ibe.encrypt_batch(eng, table, gt_table, ibe.messages, bits, ibe.t[:2]),
                 lambda: bb04ibe.decrypt_batch(eng, (d0, dj), a, b[:2], c), lambda: bb04ibe.decrypt_batch(eng, (d0[:2], dj), a, b, c),
                 lambda: bb04ibe.decrypt_batch(eng, (d0, dj[:, :7]), a, b, c)):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------------------------------------------------------ waters05 / gentry06 with gt_table
ENTRIES = ["gt_exp", "gt_mul", "g1_scalar_mul", "g2_scalar_mul", "g1_scalar_mul_base", "g1_add", "fr_neg", "fr_mul", "hash_g1_gt_gt_to_fr"]


def calls_of(oracle, run):
    """(result, [(entry, the bytes of its arguments)]) of run(engine) on a fresh recording stand-in"""
    eng = GTFixedStandIn(oracle)
    calls = recorded(eng, ENTRIES)
    res = run(eng)
    return res, [(name, [np.asarray(a).tobytes() for a in args]) for name, args in calls]


def test_waters05_gt_table_is_opt_in(oracle):
    from waters05_fixture import Instance
    inst = Instance(oracle, ["alice@example.com", "bob@example.com", "x"], tag="gtfixed")
    masks, t = waters05.identity_masks(inst.ids), inst.rows(inst.t)

    def run(gt):
        def go(eng):
            table = waters05.hash_table(eng, inst.u_prime, inst.ui)
            kw = {} if gt is False else {"gt_table": eng.GTFixedBase(inst.e_alpha) if gt else None}
            return waters05.encrypt_batch(eng, table, inst.e_alpha, inst.messages, masks, t, **kw)
        return go
    plain, plain_calls = calls_of(oracle, run(False))
    none, none_calls = calls_of(oracle, run(None))
    with_table, table_calls = calls_of(oracle, run(True))
    assert none_calls == plain_calls and [c[0] for c in plain_calls] == ["gt_exp", "gt_mul", "g1_scalar_mul_base", "g2_scalar_mul"]
    assert [c[0] for c in table_calls] == ["gt_mul", "g1_scalar_mul_base", "g2_scalar_mul"] and table_calls[1:] == plain_calls[2:]
    for got in (none, with_table):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, plain))
    assert plain[0].tobytes() == inst.c1.tobytes()


@pytest.mark.parametrize("k", [1, 3])
def test_gentry06_gt_table_is_opt_in(oracle, k):
    from gentry06_fixture import Instance
    inst = Instance(oracle, 3, k, tag="gtfixed")
    ids, s = kbytes(inst.ids), kbytes(inst.s)

    def run(gt):
        def go(eng):
            kw = {} if gt is False else {"gt_table": eng.GTFixedBase(np.concatenate([inst.e.reshape(1, 384), inst.e_gh])) if gt else None}
            res = gentry06.encrypt_batch(eng, inst.g1_alpha, inst.e, inst.e_gh, inst.messages, ids, s, **kw)
            return res, kw.get("gt_table")
        return go
    (plain, _), plain_calls = calls_of(oracle, run(False))
    (none, _), none_calls = calls_of(oracle, run(None))
    (with_table, table), table_calls = calls_of(oracle, run(True))
    assert none_calls == plain_calls and [c[0] for c in plain_calls].count("gt_exp") == (2 if k == 3 else 1)
    assert "gt_exp" not in [c[0] for c in table_calls]
    assert table.calls == [(3, 1, 1), (3, 1, 1)] + ([(3, 2, 1)] if k == 3 else [])                       # v, w's mask, and y with two terms
    for got in (none, with_table):
        assert len(got) == len(plain) == (4 if k == 3 else 3) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(got, plain))
    assert plain[1].tobytes() == inst.v.tobytes() and plain[2].tobytes() == inst.w.tobytes() and (k == 1 or plain[3].tobytes() == inst.y.tobytes())
    with pytest.raises(ValueError, match="gt_table"):
        gentry06.encrypt_batch(GTFixedStandIn(oracle), inst.g1_alpha, inst.e, inst.e_gh, inst.messages, ids, s, gt_table=GTFixedStandIn(oracle).GTFixedBase(inst.e))
