"""Host-side planner for batched Boneh-Franklin 2001 identity-based encryption (BasicIdent): SetUp (ibe/bf01_ibe/bf01_ibe.go:106-115),
KeyGenerate (:128-136), Encrypt (:156-182) and Decrypt (:200-210) for many identities / messages at once.  It is the one scheme of
the reference whose ciphertext carries BYTES, not a GT element: messages are byte strings of any length.

What is computed, with x the master key, r in Zr per ciphertext and B(.) = hash.FromGT = GT.Bytes() (384 bytes):

    SetUp         g1x = [x] g1
    KeyGenerate   Q_id = hash.ToG2(id)                sk = [x] Q_id
    Encrypt       C1 = [r] g1        gid = e(g1x, Q_id)^r        C2 = M xor B(gid)
    Decrypt       gid = e(C1, sk)                     M = C2 xor B(gid)

utils.Xor (utils/xor.go:3-16) returns a slice of the SHORTER operand's length, so a message beyond 384 bytes is cut to 384: that is
the reference's behaviour and is kept — C2 and the decrypted message come with their lengths min(len, 384), and the bytes of the
output buffer past that length are zero (engine.gt_xor_mask, ONE launch for the whole batch, messages of different lengths included).

Encrypt computes gid as e([r] g1x, Q_id): one G1 scalar multiplication of the one shared point and one pair_batch.  The reference pairs
first and raises to r in GT (:170-174).  The value is the same element of GT — e is bilinear — and a GT element has one in-memory
encoding, so B(gid) is the same 384 bytes; the G1 route is about 8x cheaper than GT.Exp (README).  The tests hold the result against
the reference's order of operations.  r = 0 gives C1 at infinity and the mask B(1), as there.

Q_id is hash.ToG2 (hash/hash_to.go): bn254.HashToG2 with hash_to.DST_STRING_G2 on the UTF-8 bytes of the identity.  The instance's DST
field ("ibe Encryption", :96) is UNUSED by the reference — nothing reads it — and is not used here.  Decrypt has no check: BasicIdent
has none, and a wrong key yields garbage, as in the reference, so there is no `ok`.

Host orchestration only, engine-agnostic (every function takes the engine: `bn254`, or a stand-in with the same names).  Host arrays
in give host arrays out; CUDA tensors in give CUDA tensors out, every step takes device rows and leaves device rows.  Messages and C2
are what engine.gt_xor_mask takes: a list of bytes, a flat buffer plus msg_off, or an [n, width] array / tensor."""
from . import _buffers as bufs, _plan

DST_STRING_G2 = b"Hash String To Element In G2"          # hash_to.DST_STRING_G2, the tag of hash.ToG2


def identities_to_g2(engine, ids, msg_off=None):
    """Q_id [n, 128] = hash.ToG2(id) for n identities: engine.hash_to_g2 with DST_STRING_G2.  ids: a list of strings (UTF-8 encoded, as
    Go's []byte(string)) and / or bytes, or a flat buffer with msg_off as hash_to_g2 takes them (host or CUDA)."""
    if msg_off is None and not _plan.is_buffer(ids):
        ids = [i.encode("utf-8") if isinstance(i, str) else bytes(i) for i in ids]
    q = engine.hash_to_g2(ids, DST_STRING_G2, msg_off)
    return bufs.view(q, bufs.nbytes(q) // 128, 128)


def public_params(engine, x):
    """g1x [64] = [x] g1 (SetUp).  x: the master key, an integer or one scalar row."""
    x = x if _plan.is_buffer(x) else _plan.scalar_rows(x)
    if bufs.nbytes(x) != 32:
        raise ValueError("x must be one scalar")
    return bufs.view(engine.g1_scalar_mul_base(bufs.flat(x)), 64)


def _qids(engine, ids, qids, like=None):
    """the identities' points [n, 128], given or hashed here, put where `like` lives"""
    if (ids is None) == (qids is None):
        raise ValueError("give the identities (ids) or their points (qids), one of the two")
    q = identities_to_g2(engine, ids) if qids is None else qids
    if bufs.nbytes(q) % 128:
        raise ValueError("qids are G2 points, rows of 128 bytes")
    q = bufs.view(q, bufs.nbytes(q) // 128, 128)
    return bufs.put(q, like) if like is not None and not bufs.is_torch(q) else q


def keygen_batch(engine, x, ids=None, qids=None):
    """sk [n, 128] = [x] Q_id for n identities (ids, hashed here) or their points (qids [n, 128]): one g2_scalar_mul."""
    q = _qids(engine, ids, qids)
    n = q.shape[0]
    x = _plan.scalars(x, q, 1, "x")
    if not n:
        return bufs.empty((0, 128), q)
    return bufs.view(engine.g2_scalar_mul(bufs.flat(q), bufs.flat(bufs.expand(bufs.view(x, 1, 32), n, 32))), n, 128)


def encrypt_batch(engine, g1x, messages, r, ids=None, qids=None, msg_off=None):
    """(C1 [n, 64], C2, c2_len [n]) for n messages to n identities with the randomness r (n scalars, or Python integers).  g1x:
    public_params.  C1 by g1_scalar_mul_base; gid = e([r] g1x, Q_id) by g1_scalar_mul of the one shared point and ONE pair_batch (see
    the module text for why this is the reference's e(g1x, Q_id)^r); C2 and c2_len by gt_xor_mask: C2 has the form of `messages`
    (for a list of bytes: the flat buffer and its offsets), c2_len[i] = min(len_i, 384), C2 beyond that is zero."""
    like = messages if _plan.is_buffer(messages) else None
    q = _qids(engine, ids, qids, like)
    n = q.shape[0]
    r = _plan.scalars(r, q, n, "r")
    g1x = _plan.public(g1x, 1, 64, q, "g1x")
    if not n:
        c2, c2_len = engine.gt_xor_mask(bufs.empty((0, 384), q), messages, msg_off)
        return bufs.empty((0, 64), q), c2, c2_len
    c1 = bufs.view(engine.g1_scalar_mul_base(r), n, 64)
    gid = engine.pair_batch(bufs.flat(engine.g1_scalar_mul(bufs.flat(g1x), r)), bufs.flat(q))
    c2, c2_len = engine.gt_xor_mask(gid, messages, msg_off)
    return c1, c2, c2_len


def encrypt_batch_seeded(engine, g1x, messages, rng, ids=None, qids=None, msg_off=None):
    """encrypt_batch with its randomness drawn on the device: rng is an rng.Randomness over the engine, everything else as there, and
    the return value is exactly encrypt_batch's on the scalars drawn.  ONE draw, r [n] — one stream id, none when n == 0 — so the
    ciphertexts are reproducible from the seed.  The scalars are of the kind the identities' points are (that of `messages` where it
    is a buffer).  The seed is key material: whoever holds it can recompute r and with it every mask."""
    q = _qids(engine, ids, qids, messages if _plan.is_buffer(messages) else None)
    r = rng.scalars(q, q.shape[0])
    return encrypt_batch(engine, g1x, messages, r, qids=q, msg_off=msg_off)


def decrypt_batch(engine, sk, C1, C2, msg_off=None):
    """(messages, lengths [n]) of n ciphertexts.  sk: one key for all of them ([128] or [1, 128]) — multi_pair_fixed_q(C1, sk) with ONE
    shared G2 point, whose lines are computed once for the batch — or one per ciphertext ([n, 128]) — pair_batch; then gt_xor_mask.
    C2 as encrypt_batch returns it (a (buffer, offsets) pair is taken apart here) or in any form gt_xor_mask takes; messages has its
    form, lengths[i] = min(len_i, 384).  There is no check to fail: a wrong key gives other bytes."""
    if isinstance(C2, tuple) and msg_off is None:
        C2, msg_off = C2
    n = bufs.nbytes(C1) // 64
    if bufs.nbytes(C1) != n * 64:
        raise ValueError("C1 holds G1 points, rows of 64 bytes")
    C1 = bufs.view(C1, n, 64)
    shared = bufs.nbytes(sk) == 128
    sk = _plan.public(sk, 1 if shared else n, 128, C1, "sk")
    if not n:
        return engine.gt_xor_mask(bufs.empty((0, 384), C1), C2, msg_off)
    gid = engine.multi_pair_fixed_q(bufs.flat(C1), bufs.flat(sk)) if shared else engine.pair_batch(bufs.flat(C1), bufs.flat(sk))
    return engine.gt_xor_mask(gid, C2, msg_off)
