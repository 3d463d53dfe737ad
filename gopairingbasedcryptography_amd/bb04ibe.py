"""Host-side planner for batched Boneh-Boyen 2004 identity-based encryption with bit-string identities (ibe/bb04_ibe/bb04_ibe.go):
SetUp (:94-134), KeyGenerate (:138-170), Encrypt (:173-206) and Decrypt (:210-241) for many identities / messages at once.

What is computed.  An identity is the n = 256 bits a_0 .. a_255 of SHA-256(string), most significant bit of every byte first
(NewBB04IBEIdentity, :245-271); the public parameters hold two G2 points per bit, u[j][0] and u[j][1], and bit j of an identity picks
u[j][a_j].  With the master key alpha and the randomness r_j, t in Zr:

    KeyGenerate   d_j = [r_j] g1  (j < n)        d0 = g2^alpha + sum_j [r_j] u[j][a_j]
    Encrypt       a = M e(g1^alpha, g2)^t        b = [t] g1          c_j = [t] u[j][a_j]  (j < n)
    Decrypt       M = a prod_j e(d_j, c_j) / e(b, d0)  = a * Pair([d_0 .. d_(n-1), -b], [c_0 .. c_(n-1), d0])

The 2 n points live in ONE G2 fixed-base table (u_table: engine.FixedBase, 2 MB per point), ordered u[0][0], u[0][1], u[1][0], ...,
so bit j of an identity is the index 2 j + a_j (index_rows) and both loops are indexed sums over that table: c_j with one term per
output, the sum of d0 in groups of 16 terms (the table's limit per output, padded with INDEX_NONE) followed by g2_sum_segments.
e(g1^alpha, g2) depends on the public parameters alone: public_pairing computes it once, the reference on every Encrypt, and a GT
fixed-base table over it (gt_table: engine.GTFixedBase) gives e(g1^alpha, g2)^t in 32 products per message.  The quotient of Decrypt
folds into the pairing exactly — e(b, d0)^-1 = e(-b, d0) as Fp12 elements — so a ciphertext costs one multi-pairing segment of n + 1
pairs (one final exponentiation) and one GT multiplication.

The identity length is a parameter (`length`, the number of bit positions; the reference's constant n = 256 is the default) and is
otherwise read from the shapes.  Host orchestration only, engine-agnostic (every function takes the engine: `bn254`, or a stand-in with
the same names).  The randomness comes in as arguments (scalar rows, or Python integers); the *_seeded forms draw it from an
rng.Randomness.  Host arrays in give host arrays out; CUDA tensors in give CUDA tensors out."""
import hashlib

import numpy as np

from . import _buffers as bufs, _plan

ID_BITS = 256                    # n of the reference
GROUP = 16                       # terms per output of FixedBase.indexed


def _length(length):
    if not isinstance(length, (int, np.integer)) or isinstance(length, bool) or not 1 <= length <= ID_BITS:
        raise ValueError("the identity length must be in 1 .. %d bits (got %s)" % (ID_BITS, length))
    return int(length)


def identity_bits(strings, length=ID_BITS):
    """[n, length] uint8 of 0 / 1: bit j of an identity is (digest[j // 8] >> (7 - j % 8)) & 1 of SHA-256(string), the first `length`
    of them.  An empty string is refused, as the reference refuses it."""
    length, rows = _length(length), []
    for s in strings:
        b = s.encode() if isinstance(s, str) else bytes(s)
        if not b:
            raise ValueError("identity string cannot be empty")
        rows.append(hashlib.sha256(b).digest())
    digests = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, 32)
    return np.ascontiguousarray(bufs.unpack_bits(digests)[:, :length])


def identity_bits_device(engine, strings_or_buffer, msg_off=None, length=ID_BITS):
    """identity_bits through engine.sha256: the digests computed on the device and unpacked where they are.  A list of identity strings
    (or bytes), or the concatenated bytes with msg_off as engine.sha256 takes them — host arrays give a host array, CUDA tensors a CUDA
    tensor that goes into the batch functions as it is.  An empty string in a list is refused; offsets are not inspected."""
    length = _length(length)
    if msg_off is None:
        strings_or_buffer = [s.encode() if isinstance(s, str) else bytes(s) for s in strings_or_buffer]
        if not all(strings_or_buffer):
            raise ValueError("identity string cannot be empty")
    digests = engine.sha256(strings_or_buffer, msg_off)
    return bufs.unpack_bits(bufs.view(digests, -1, 32))[:, :length]


def index_rows(bits):
    """[n, length] indices into u_table, 2 j + a_j for bit j, of the kind FixedBase.indexed takes: uint32 on the host, int32 in a
    tensor.  Any non-zero entry of `bits` counts as 1."""
    if len(bits.shape) != 2:
        raise ValueError("identity bits are an [n, length] array of 0 / 1")
    even = np.arange(0, 2 * bits.shape[1], 2)
    if bufs.is_torch(bits):
        return (bits != 0).int() + bufs.put(even.astype(np.int32), bits)
    return (np.asarray(bits) != 0).astype(np.uint32) + even.astype(np.uint32)


def public_params(engine, alpha, u_scalars):
    """(g1_alpha [64], g2_alpha [128], uij [2 length, 128]) (NewBB04IBEInstance and SetUp): [alpha] g1, [alpha] g2 — the latter stays
    with the key generator — and u[j][b] = [u_scalars[2 j + b]] g2, the reference's loop order.  alpha: an integer or one scalar row;
    u_scalars: 2 x length of them."""
    alpha = alpha if _plan.is_buffer(alpha) else _plan.scalar_rows(alpha)
    u = u_scalars if _plan.is_buffer(u_scalars) else _plan.scalar_rows(u_scalars)
    m = bufs.nbytes(u) // 32
    if bufs.nbytes(alpha) != 32 or bufs.nbytes(u) != m * 32 or m % 2 or not 2 <= m <= 2 * ID_BITS:
        raise ValueError("alpha must be one scalar and u_scalars two per identity bit")
    return (bufs.view(engine.g1_scalar_mul_base(bufs.flat(alpha)), 64), bufs.view(engine.g2_scalar_mul_base(bufs.flat(alpha)), 128),
            bufs.view(engine.g2_scalar_mul_base(bufs.flat(u)), m, 128))


def public_pairing(engine, g1_alpha):
    """e(g1^alpha, g2) [384]: one pairing per public parameters, what gt_table is built over"""
    return bufs.view(engine.pair_batch(bufs.flat(g1_alpha), bufs.put(engine.generators()[1], g1_alpha)), 384)


def u_table(engine, uij):
    """the 2 x length points u[j][b] as a G2 fixed-base table (engine.FixedBase); table.close() frees it"""
    m = bufs.nbytes(uij) // 128
    if bufs.nbytes(uij) != m * 128 or m % 2 or not 2 <= m <= 2 * ID_BITS:
        raise ValueError("uij holds two G2 points per identity bit")
    return engine.FixedBase(uij, g2=True)


def _bits(table, bits):
    if len(bits.shape) != 2 or 2 * bits.shape[1] != table.nbase:
        raise ValueError("identity bits must be [n, %d], one per pair of points of the table" % (table.nbase // 2))
    return bits.shape[0], bits.shape[1]


def keygen_batch(engine, table, g2_alpha, bits, r):
    """(d0 [n, 128], dj [n, length, 64]) for n identities (bits [n, length]) with the randomness r (n x length scalars).  dj by ONE
    g1_scalar_mul_base; the sum of d0 by table.indexed over ceil(length / 16) groups of 16 terms per identity, the last padded with
    INDEX_NONE, g2_sum_segments over an identity's groups, and g2_add with the one shared g2^alpha."""
    n, L = _bits(table, bits)
    r = _plan.scalars(r, bits, n * L, "r")
    ga = bufs.flat(_plan.public(g2_alpha, 1, 128, bits, "g2_alpha"))
    if not n:
        return bufs.empty((0, 128), bits), bufs.empty((0, L, 64), bits)
    dj = bufs.view(engine.g1_scalar_mul_base(r), n, L, 64)
    groups = -(-L // GROUP)
    index, k, pad = index_rows(bits), bufs.view(r, n, L, 32), groups * GROUP - L
    if pad:
        none = np.full((n, pad), _plan.INDEX_NONE, dtype=np.uint32)
        index = bufs.cat([index, bufs.put(none.view(np.int32), bits) if bufs.is_torch(bits) else none], 1)
        k = bufs.cat([k, bufs.zeros((n, pad, 32), bits)], 1)
    partial, _ = table.indexed(bufs.flat(index), bufs.flat(k), terms=GROUP)
    total = partial if groups == 1 else engine.g2_sum_segments(bufs.flat(partial), _plan.segments(n, groups))
    return bufs.view(engine.g2_add(bufs.flat(total), ga), n, 128), dj


def keygen_batch_seeded(engine, table, g2_alpha, bits, rng):
    """keygen_batch with its randomness drawn on the device: ONE draw, r [n, length] — one stream id, none when n == 0 — of the kind
    the bits are.  The seed is key material."""
    n, L = _bits(table, bits)
    return keygen_batch(engine, table, g2_alpha, bits, rng.scalars(bits, n, L))


def encrypt_batch(engine, table, gt_table, messages, bits, t):
    """(a [n, 384], b [n, 64], c [n, length, 128]) for n messages (GT elements, [n, 384]) to n identities (bits [n, length]) with the
    randomness t (n scalars).  gt_table: an engine.GTFixedBase whose base 0 is e(g1^alpha, g2).  c by table.indexed with ONE term per
    output (n x length outputs, t repeated along an identity), b by g1_scalar_mul_base, a = gt_mul(gt_table.pow(t), M)."""
    n, L = _bits(table, bits)
    t = _plan.scalars(t, bits, n, "t")
    if bufs.nbytes(messages) != n * 384 or bufs.is_torch(messages) != bufs.is_torch(bits):
        raise ValueError("need n = %d messages of the kind the bits are" % n)
    if not n:
        return bufs.empty((0, 384), bits), bufs.empty((0, 64), bits), bufs.empty((0, L, 128), bits)
    a = engine.gt_mul(bufs.flat(gt_table.pow(t)), bufs.flat(messages))
    b = engine.g1_scalar_mul_base(t)
    c, _ = table.indexed(bufs.flat(index_rows(bits)), bufs.flat(bufs.expand(bufs.view(t, n, 1, 32), n, L, 32)), terms=1)
    return bufs.view(a, n, 384), bufs.view(b, n, 64), bufs.view(c, n, L, 128)


def encrypt_batch_seeded(engine, table, gt_table, messages, bits, rng):
    """encrypt_batch with its randomness drawn on the device: ONE draw, t [n] — one stream id, none when n == 0 — of the kind the
    bits are; the return value is exactly encrypt_batch's on the scalars drawn.  The seed is key material."""
    return encrypt_batch(engine, table, gt_table, messages, bits, rng.scalars(bits, bits.shape[0]))


def decrypt_batch(engine, key, a, b, c):
    """messages [n, 384] of n ciphertexts under key = (d0, dj): one key for all of them ([128], [length, 64]) or one per ciphertext
    ([n, 128], [n, length, 64]).  -b by g1_sub from the point at infinity, ONE multi_pair segment of length + 1 pairs per ciphertext —
    (d_j, c_j) for every j, then (-b, d0) — and gt_mul with a.  A key of another identity gives some other GT element, as in the
    reference."""
    d0, dj = key
    bufs.device_of(a, b, c)
    n = bufs.nbytes(a) // 384
    if bufs.nbytes(a) != n * 384 or bufs.nbytes(b) != n * 64 or (n and bufs.nbytes(c) % (n * 128)):
        raise ValueError("a, b, c must hold n GT elements, n G1 points and n rows of G2 points")
    a = bufs.view(a, n, 384)
    if not n:
        return a
    L = bufs.nbytes(c) // (n * 128)
    c, b = bufs.view(c, n, L, 128), bufs.view(b, n, 64)
    d0, dj = _plan.per_item(d0, n, 1, 128, a, "d0"), _plan.per_item(dj, n, L, 64, a, "dj")
    neg_b = bufs.view(engine.g1_sub(bufs.zeros((n * 64,), a), bufs.flat(b)), n, 1, 64)
    P = bufs.flat(bufs.cat([dj, neg_b], 1))                                       # [n, L + 1, 64]
    Q = bufs.flat(bufs.cat([c, d0], 1))                                           # [n, L + 1, 128]
    pairs = engine.multi_pair(P, Q, _plan.segments(n, L + 1))
    return bufs.view(engine.gt_mul(bufs.flat(a), bufs.flat(pairs)), n, 384)
