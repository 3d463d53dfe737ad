"""The Boneh-Boyen IBE planners on the MI355X (run with -m gpu): bb04sibe.py and bb04ibe.py over the real engine, host arrays and CUDA
tensors.  Encrypt components are held against the oracle's pair + gt_exp + gt_mul (and its scalar multiplications), keys against ONE
oracle multiplication by the exponent the reference's sequence arrives at, Decrypt recovers every message, and the one-key and the
key-per-ciphertext forms agree.  BB04 IBE runs at the reference's identity length 256 with 3 identities and at 16 with 65 (more than two
wavefronts of lane pairs in the GT table's kernel).  The gt_table option of waters05 and gentry06 gives the bytes of the gt_exp route."""
import numpy as np
import pytest

import bn254_py as o
from sw05_fixture import kbytes
from gopairingbasedcryptography_amd import bb04ibe, bb04sibe, gentry06, waters05

pytestmark = pytest.mark.gpu
R = o.R
G1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
G2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)


def sc(tag, i=0):
    return o.bench_scalar("bb04-gpu-" + tag, i)


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def messages_of(oracle, n, tag):
    e = np.asarray(oracle.pair_batch(G1, G2)).reshape(384)
    return np.asarray(oracle.gt_exp(np.tile(e, (n, 1)), kbytes([sc(tag + "msg", i) for i in range(n)]), threads=8)).reshape(n, 384)


@pytest.mark.parametrize("on_device", [False, True])
def test_sibe_round_trip(eng, oracle, on_device):
    n = 33
    put = to_dev if on_device else (lambda a: a)
    x, y = sc("x"), sc("y")
    ids, r, s = ([sc(name, i) for i in range(n)] for name in ("id", "r", "s"))
    ids[5] = (-(x + r[5] * y)) % R                                             # ID + x + r y = 0: the key is the point at infinity
    M = messages_of(oracle, n, "sibe")
    X, Y = bb04sibe.public_params(eng, x, y)
    e = bb04sibe.public_pairing(eng)
    assert e.tobytes() == np.asarray(oracle.pair_batch(G1, G2)).tobytes()
    table = eng.GTFixedBase(put(e))
    k = bb04sibe.keygen_batch(eng, x, y, put(kbytes(ids)), put(kbytes(r)))
    inv = [pow(d, -1, R) if d else 0 for d in ((i + x + ri * y) % R for i, ri in zip(ids, r))]
    assert host(k).tobytes() == np.asarray(oracle.g2_scalar_mul(G2, kbytes(inv), threads=8)).tobytes() and not host(k)[5].any()
    a, b, c = bb04sibe.encrypt_batch(eng, (X, Y), table, put(M), put(kbytes(ids)), put(kbytes(s)))
    assert host(a).tobytes() == np.asarray(oracle.g1_scalar_mul(G1, kbytes([si * (i + x) for si, i in zip(s, ids)]), threads=8)).tobytes()
    assert host(b).tobytes() == np.asarray(oracle.g1_scalar_mul(G1, kbytes([si * y for si in s]), threads=8)).tobytes()
    assert host(c).tobytes() == np.asarray(oracle.gt_mul(oracle.gt_exp(np.tile(e, (n, 1)), kbytes(s), threads=8), M)).tobytes()
    if on_device:
        assert all(v.is_cuda for v in (k, a, b, c))
    good = [i for i in range(n) if i != 5]
    take = (lambda v: v[to_dev(np.array(good))]) if on_device else (lambda v: v[good])
    m = bb04sibe.decrypt_batch(eng, take(a), take(b), take(c), take(put(kbytes(r).reshape(n, 32))), take(k))
    assert host(m).tobytes() == M[good].tobytes()
    # n messages to ONE identity: one key for all, and the same key per ciphertext
    k1 = bb04sibe.keygen_batch(eng, x, y, [ids[0]], [r[0]])
    a, b, c = bb04sibe.encrypt_batch(eng, (X, Y), table, put(M), put(kbytes([ids[0]] * n)), put(kbytes(s)))
    one = bb04sibe.decrypt_batch(eng, a, b, c, r[0], k1[0])
    each = bb04sibe.decrypt_batch(eng, a, b, c, put(kbytes([r[0]] * n)), put(np.tile(k1[0], (n, 1))))
    assert host(one).tobytes() == host(each).tobytes() == M.tobytes()
    wrong = bb04sibe.decrypt_batch(eng, a, b, c, r[1], host(k)[1])
    assert not (host(wrong) == M).all(1).any()
    table.close()


@pytest.mark.parametrize("L,n,on_device", [(256, 3, True), (16, 65, True), (16, 65, False)])
def test_ibe_round_trip(eng, oracle, L, n, on_device):
    put = to_dev if on_device else (lambda a: a)
    tag = "ibe%d-" % L
    alpha, u_k = sc(tag + "alpha"), [sc(tag + "u", i) for i in range(2 * L)]
    ids = ["user-%d@example.com" % i for i in range(n)]
    r = [[sc(tag + "r", i * L + j) for j in range(L)] for i in range(n)]
    t = [sc(tag + "t", i) for i in range(n)]
    M = messages_of(oracle, n, tag)
    g1a, g2a, uij = bb04ibe.public_params(eng, alpha, u_k)
    assert uij.tobytes() == np.asarray(oracle.g2_scalar_mul(G2, kbytes(u_k), threads=8)).tobytes()
    e_alpha = bb04ibe.public_pairing(eng, g1a)
    assert e_alpha.tobytes() == np.asarray(oracle.pair_batch(g1a, G2)).tobytes()
    table, gt_table = bb04ibe.u_table(eng, put(uij)), eng.GTFixedBase(put(e_alpha))
    bits_host = bb04ibe.identity_bits(ids, L)
    bits = bb04ibe.identity_bits_device(eng, [s.encode() for s in ids], length=L) if not on_device else \
        bb04ibe.identity_bits_device(eng, to_dev(np.frombuffer("".join(ids).encode(), dtype=np.uint8)),
                                     to_dev(np.cumsum([0] + [len(s) for s in ids]).astype(np.int64)), length=L).contiguous()
    assert host(bits).tolist() == bits_host.tolist()
    picked = [[u_k[2 * j + int(b)] for j, b in enumerate(row)] for row in bits_host]                    # log_g2 of u[j][a_j]
    d0, dj = bb04ibe.keygen_batch(eng, table, g2a, bits, put(kbytes([v for row in r for v in row])))
    assert host(dj).tobytes() == np.asarray(oracle.g1_scalar_mul(G1, kbytes([v for row in r for v in row]), threads=8)).tobytes()
    assert host(d0).tobytes() == np.asarray(oracle.g2_scalar_mul(G2, kbytes([alpha + sum(a * b for a, b in zip(ri, ui)) for ri, ui in zip(r, picked)]), threads=8)).tobytes()
    a, b, c = bb04ibe.encrypt_batch(eng, table, gt_table, put(M), bits, put(kbytes(t)))
    assert tuple(c.shape) == (n, L, 128)
    assert host(a).tobytes() == np.asarray(oracle.gt_mul(oracle.gt_exp(np.tile(e_alpha, (n, 1)), kbytes(t), threads=8), M)).tobytes()
    assert host(b).tobytes() == np.asarray(oracle.g1_scalar_mul(G1, kbytes(t), threads=8)).tobytes()
    assert host(c).tobytes() == np.asarray(oracle.g2_scalar_mul(G2, kbytes([ti * u for ti, ui in zip(t, picked) for u in ui]), threads=8)).tobytes()
    if on_device:
        assert all(v.is_cuda for v in (d0, dj, a, b, c))
    m = bb04ibe.decrypt_batch(eng, (d0, dj), a, b, c)                                                   # a key per ciphertext
    assert host(m).tobytes() == M.tobytes()
    wrong = bb04ibe.decrypt_batch(eng, (host(d0)[1], host(dj)[1]), a[:1], b[:1], c[:1])                 # the key of another identity
    assert host(wrong).tobytes() != M[:1].tobytes()
    # every message to identity 0: one key for all, and the same key per ciphertext
    same = put(np.tile(bits_host[0], (n, 1)))
    a, b, c = bb04ibe.encrypt_batch(eng, table, gt_table, put(M), same, put(kbytes(t)))
    one = bb04ibe.decrypt_batch(eng, (host(d0)[0], host(dj)[0]), a, b, c)
    each = bb04ibe.decrypt_batch(eng, (put(np.tile(host(d0)[0], (n, 1))), put(np.tile(host(dj)[0], (n, 1, 1)))), a, b, c)
    assert host(one).tobytes() == host(each).tobytes() == M.tobytes()
    table.close()
    gt_table.close()


@pytest.mark.parametrize("on_device", [False, True])
def test_waters05_and_gentry06_with_a_gt_table(eng, oracle, on_device):
    """the gt_table option on the real engine: every byte of Encrypt equals the gt_exp route's"""
    from gentry06_fixture import Instance as Gentry
    from waters05_fixture import Instance as Waters
    put = to_dev if on_device else (lambda a: a)
    ids = ["id-%d" % i for i in range(33)]
    w = Waters(oracle, ids, tag="gtfixed-gpu")
    masks, t = put(waters05.identity_masks(ids)), put(w.rows(w.t))
    hash_table, gt_table = waters05.hash_table(eng, put(w.u_prime), put(w.ui)), eng.GTFixedBase(put(w.e_alpha))
    plain = waters05.encrypt_batch(eng, hash_table, w.e_alpha, put(w.messages), masks, t)
    fixed = waters05.encrypt_batch(eng, hash_table, w.e_alpha, put(w.messages), masks, t, gt_table=gt_table)
    assert all(host(x).tobytes() == host(y).tobytes() for x, y in zip(fixed, plain)) and host(plain[0]).tobytes() == w.c1.tobytes()
    hash_table.close()
    gt_table.close()
    for k in (1, 3):
        g = Gentry(oracle, 33, k, tag="gtfixed-gpu")
        gt_table = eng.GTFixedBase(put(np.concatenate([g.e.reshape(1, 384), g.e_gh])))
        args = (eng, g.g1_alpha, g.e, g.e_gh, put(g.messages), put(kbytes(g.ids)), put(kbytes(g.s)))
        plain, fixed = gentry06.encrypt_batch(*args), gentry06.encrypt_batch(*args, gt_table=gt_table)
        assert len(fixed) == len(plain) == (4 if k == 3 else 3) and all(host(x).tobytes() == host(y).tobytes() for x, y in zip(fixed, plain))
        assert host(plain[1]).tobytes() == g.v.tobytes() and (k == 1 or host(plain[3]).tobytes() == g.y.tobytes())
        gt_table.close()
