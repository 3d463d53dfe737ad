"""Host-side planner for batched Boneh-Boyen 2004 selective-ID identity-based encryption (ibe/bb04_sibe/bb04_sibe.go): SetUp (:109-120),
KeyGenerate (:133-163), Encrypt (:177-203) and Decrypt (:217-231) for many identities / messages at once.

What is computed, with the master key (x, y), an identity ID and the randomness r, s in Zr:

    SetUp         X = [x] g1            Y = [y] g1
    KeyGenerate   k = [1 / (ID + x + r y)] g2                              the key is (r, k)
    Encrypt       a = [s ID] g1 + [s] X     b = [s] Y     c = e(g1, g2)^s M
    Decrypt       M = c / e(a + [r] b, k)   = c * e(-(a + [r] b), k)

e(g1, g2) depends on nothing: public_pairing computes it once, the reference on every Encrypt, and a GT fixed-base table over it
(engine.GTFixedBase, gt_table) turns e(g1, g2)^s into 32 products per message — table.pow(s) — where gt_exp on a replicated base
squares 252 times.  The quotient of Decrypt folds into the pairing exactly — e(P, Q)^-1 = e(-P, Q) as Fp12 elements, as in
waters05.decrypt_batch — so a ciphertext costs one pairing and one GT multiplication, no GT inversion.  fr.Element.Inverse(0) is 0 in
gnark, so the key of an identity with ID + x + r y = 0 is the point at infinity, as in the reference; nothing is refused.

Host orchestration only, engine-agnostic (every function takes the engine: `bn254`, or a stand-in with the same names).  The
randomness r / s comes in as arguments (scalar rows, or Python integers); the *_seeded forms draw it from an rng.Randomness.  Host
arrays in give host arrays out; CUDA tensors in give CUDA tensors out."""
from . import _buffers as bufs, _plan


def _repeat(x, n):
    """one scalar row once per item: [n * 32], flat"""
    return bufs.flat(bufs.expand(bufs.view(x, 1, 32), n, 32))


def public_params(engine, x, y):
    """(X [64], Y [64]) = ([x] g1, [y] g1) (SetUp).  x, y: the master key, integers or one scalar row each."""
    xy = [v if _plan.is_buffer(v) else _plan.scalar_rows(v) for v in (x, y)]
    if any(bufs.nbytes(v) != 32 for v in xy):
        raise ValueError("x and y must be one scalar each")
    return tuple(bufs.view(engine.g1_scalar_mul_base(bufs.flat(v)), 64) for v in xy)


def public_pairing(engine):
    """e(g1, g2) [384]: one pairing per process, what gt_table is built over (engine.GTFixedBase(public_pairing(engine)))"""
    g1, g2 = engine.generators()
    return bufs.view(engine.pair_batch(g1, g2), 384)


def keygen_batch(engine, x, y, ids, r):
    """k [n, 128] for n identities (scalars) with the randomness r (n scalars): fr_mul r y, fr_add x, fr_add ID, fr_inverse,
    g2_scalar_mul_base — the reference's operations in its order.  The key of identity i is (r[i], k[i]); where ID + x + r y = 0 the
    inverse is 0 and k[i] the point at infinity (all zero), as gnark computes it."""
    ids = ids if _plan.is_buffer(ids) else _plan.scalar_rows(ids)
    n = bufs.nbytes(ids) // 32
    ids, r = _plan.scalars(ids, ids, n, "ids"), _plan.scalars(r, ids, n, "r")
    x, y = _plan.scalars(x, ids, 1, "x"), _plan.scalars(y, ids, 1, "y")
    if not n:
        return bufs.empty((0, 128), ids)
    d = engine.fr_add(engine.fr_add(engine.fr_mul(r, _repeat(y, n)), _repeat(x, n)), ids)
    return bufs.view(engine.g2_scalar_mul_base(engine.fr_inverse(bufs.flat(d))), n, 128)


def keygen_batch_seeded(engine, x, y, ids, rng):
    """(r [n, 32], k [n, 128]): keygen_batch with its randomness drawn on the device.  ONE draw, r [n] — one stream id, none when
    n == 0.  The seed is key material."""
    ids = ids if _plan.is_buffer(ids) else _plan.scalar_rows(ids)
    r = rng.scalars(ids, bufs.nbytes(ids) // 32)
    return r, keygen_batch(engine, x, y, ids, r)


def encrypt_batch(engine, pp, gt_table, messages, ids, s):
    """(a [n, 64], b [n, 64], c [n, 384]) for n messages (GT elements, [n, 384]) to n identities (scalars) with the randomness s.
    pp = (X, Y): public_params; gt_table: an engine.GTFixedBase whose base 0 is e(g1, g2).  a by fr_mul, g1_scalar_mul_base,
    g1_scalar_mul of the one shared X and g1_add; b by g1_scalar_mul of the one shared Y; c = gt_mul(gt_table.pow(s), M)."""
    n = bufs.nbytes(messages) // 384
    if bufs.nbytes(messages) != n * 384:
        raise ValueError("messages are GT elements, rows of 384 bytes")
    messages = bufs.view(messages, n, 384)
    ids, s = _plan.scalars(ids, messages, n, "ids"), _plan.scalars(s, messages, n, "s")
    X, Y = (_plan.public(p, 1, 64, messages, what) for p, what in zip(pp, ("X", "Y")))
    if not n:
        return bufs.empty((0, 64), messages), bufs.empty((0, 64), messages), messages
    a = engine.g1_add(engine.g1_scalar_mul_base(engine.fr_mul(s, ids)), engine.g1_scalar_mul(bufs.flat(X), s))
    b = engine.g1_scalar_mul(bufs.flat(Y), s)
    c = engine.gt_mul(bufs.flat(gt_table.pow(s)), bufs.flat(messages))
    return bufs.view(a, n, 64), bufs.view(b, n, 64), bufs.view(c, n, 384)


def encrypt_batch_seeded(engine, pp, gt_table, messages, ids, rng):
    """encrypt_batch with its randomness drawn on the device: ONE draw, s [n] — one stream id, none when n == 0 — of the kind the
    messages are; the return value is exactly encrypt_batch's on the scalars drawn.  The seed is key material."""
    return encrypt_batch(engine, pp, gt_table, messages, ids, rng.scalars(messages, bufs.nbytes(messages) // 384))


def decrypt_batch(engine, a, b, c, r, k):
    """messages [n, 384] of n ciphertexts under the key (r, k): one key for all of them ([32], [128]) or one per ciphertext ([n, 32],
    [n, 128]).  a + [r] b by g1_scalar_mul and g1_add, its negative by g1_sub from the point at infinity, ONE pair_batch (a pair per
    item), then gt_mul with c.  There is no check to fail: a key of another identity gives some other GT element, as in the reference."""
    bufs.device_of(a, b, c)
    n = bufs.nbytes(c) // 384
    if bufs.nbytes(c) != n * 384 or bufs.nbytes(a) != n * 64 or bufs.nbytes(b) != n * 64:
        raise ValueError("a, b, c must hold n G1, G1 and GT elements")
    c = bufs.view(c, n, 384)
    r = r if _plan.is_buffer(r) else _plan.scalar_rows(r)
    r, k = _plan.per_item(r, n, 1, 32, c, "r"), _plan.per_item(k, n, 1, 128, c, "k")
    if not n:
        return c
    abr = engine.g1_add(bufs.flat(bufs.view(a, n, 64)), engine.g1_scalar_mul(bufs.flat(bufs.view(b, n, 64)), bufs.flat(r)))
    neg = engine.g1_sub(bufs.zeros((n * 64,), c), bufs.flat(abr))
    return bufs.view(engine.gt_mul(bufs.flat(c), bufs.flat(engine.pair_batch(bufs.flat(neg), bufs.flat(k)))), n, 384)
