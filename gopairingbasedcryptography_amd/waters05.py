"""Host-side planner for batched Waters 2005 identity-based encryption (ibe/waters05_ibe/waters05_ibe.go): KeyGenerate (:163-193),
Encrypt (:206-244) and Decrypt (:257-279) for many identities / messages at once.

What is computed.  An identity is the 256 bits of SHA-256(string), most significant bit of every byte first (NewWaters05IBEIdentity,
:290-315) — as 32 mask bytes that is the digest itself.  Both KeyGenerate and Encrypt start with the Waters hash

    H(id) = U' + sum_{Id[i] = 1} U_i          up to 256 G2Affine.Add in the reference, each with an inversion of its own

which here is ONE engine.SubsetTable over the 256 public U_i with offset U' (2 MiB, built once per public parameters) and one
table.sum per batch: 32 mixed additions per identity, from its 32 bytes.  Then

    KeyGenerate   d2 = [r] g1                      d1 = g2^alpha + [r] H(id)
    Encrypt       c1 = M * e(g1^alpha, g2)^t       c2 = [t] g1          c3 = [t] H(id)
    Decrypt       M  = c1 * e(d2, c3) / e(c2, d1)  = c1 * Pair([d2, -c2], [c3, d1])

The quotient of Decrypt folds into the pairing exactly — e(c2, d1)^-1 = e(-c2, d1) as Fp12 elements — so a ciphertext costs one
2-pair multi-pairing segment (one final exponentiation) and one GT multiplication, no GT inversion.

Host orchestration only, engine-agnostic (every function takes the engine: `bn254`, or a stand-in with the same names).  The
randomness r / t comes in as arguments (scalar rows, or Python integers).  Host arrays in give host arrays out; CUDA tensors in give
CUDA tensors out and nothing but the shared points (g2^alpha, e(g1^alpha, g2)) and integer scalars travels to the device."""
import hashlib

import numpy as np

from . import _buffers as bufs, _plan

ID_BITS, ID_BYTES = 256, 32


def identity_masks(strings):
    """SHA-256 of every identity string as an [n, 32] uint8 array: bit 7 - t of byte w is Id[8 w + t] of NewWaters05IBEIdentity.
    An empty string is refused, as the reference refuses it.  Callers that hold digests pass them to the batch functions directly."""
    rows = []
    for s in strings:
        b = s.encode() if isinstance(s, str) else bytes(s)
        if not b:
            raise ValueError("identity string cannot be empty")
        rows.append(hashlib.sha256(b).digest())
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, ID_BYTES).copy()


def identity_masks_device(engine, strings_or_buffer, msg_off=None):
    """identity_masks through engine.sha256: the [n, 32] digests computed on the device.  A list of identity strings (or bytes), or the
    concatenated bytes with msg_off as engine.sha256 takes them — host arrays give a host array, CUDA tensors a CUDA tensor that goes
    into the batch functions as it is.  An empty string in a list is refused, as the reference refuses it; offsets are not inspected."""
    if msg_off is not None:
        return engine.sha256(strings_or_buffer, msg_off)
    msgs = [s.encode() if isinstance(s, str) else bytes(s) for s in strings_or_buffer]
    if not all(msgs):
        raise ValueError("identity string cannot be empty")
    return engine.sha256(msgs)


def hash_table(engine, u_prime, ui):
    """the Waters hash as a table: engine.SubsetTable over the 256 U_i ([256, 128]) with offset U' ([128]); table.close() frees it"""
    if bufs.nbytes(ui) != ID_BITS * 128 or bufs.nbytes(u_prime) != 128:
        raise ValueError("need 256 points U_i and one point U' in G2")
    return engine.SubsetTable(ui, offset=u_prime, g2=True)


def _masks(masks):
    if bufs.nbytes(masks) % ID_BYTES:
        raise ValueError("identity masks are rows of 32 bytes")
    return bufs.view(masks, -1, ID_BYTES)


def keygen_batch(engine, table, g2_alpha, masks, r):
    """(d1 [n, 128], d2 [n, 64]) for n identities: d2 = [r] g1 (g1_scalar_mul_base), d1 = g2^alpha + [r] H(id) (table.sum,
    g2_scalar_mul, g2_add with the one shared g2^alpha)."""
    masks = _masks(masks)
    n = masks.shape[0]
    r = _plan.scalars(r, masks, n, "r")
    ga = bufs.flat(_plan.public(g2_alpha, 1, 128, masks, "g2_alpha"))
    d2 = engine.g1_scalar_mul_base(r)
    h = table.sum(masks)
    d1 = engine.g2_add(engine.g2_scalar_mul(bufs.flat(h), r), ga)
    return bufs.view(d1, n, 128), bufs.view(d2, n, 64)


def encrypt_batch(engine, table, e_alpha, messages, masks, t, gt_table=None):
    """(c1 [n, 384], c2 [n, 64], c3 [n, 128]) for n messages (GT elements, [n, 384]) to n identities: e_alpha = e(g1^alpha, g2), one
    GT element, is replicated and raised to t by gt_exp, c1 = gt_mul(that, M); c2 = [t] g1; c3 = [t] H(id).
    gt_table: an engine.GTFixedBase whose base 0 is e_alpha; with it e_alpha^t is gt_table.pow(t), 32 products per message and no
    squarings, and the bytes are the same.  Without it (the default) the calls are the ones above."""
    masks = _masks(masks)
    n = masks.shape[0]
    t = _plan.scalars(t, masks, n, "t")
    if bufs.nbytes(messages) != n * 384 or bufs.is_torch(messages) != bufs.is_torch(masks):
        raise ValueError("need n = %d messages of the kind the masks are" % n)
    if gt_table is None:
        c1 = _plan.blind(engine, _plan.public(e_alpha, 1, 384, masks, "e_alpha"), t, messages, n)
    else:
        c1 = engine.gt_mul(bufs.flat(gt_table.pow(t)), bufs.flat(messages))
    c2 = engine.g1_scalar_mul_base(t)
    c3 = engine.g2_scalar_mul(bufs.flat(table.sum(masks)), t)
    return bufs.view(c1, n, 384), bufs.view(c2, n, 64), bufs.view(c3, n, 128)


def decrypt_batch(engine, key, c1, c2, c3):
    """messages [n, 384] of n ciphertexts under key = (d1, d2): one key for all of them ([128], [64]) or one per ciphertext
    ([n, 128], [n, 64]).  M = c1 * e(d2, c3) * e(-c2, d1): -c2 by g1_sub from the point at infinity, one multi_pair segment of two
    pairs per ciphertext, then gt_mul.  A key of another identity gives some other GT element, as in the reference."""
    d1, d2 = key
    bufs.device_of(c1, c2, c3)
    n = bufs.nbytes(c1) // 384
    if bufs.nbytes(c1) != n * 384 or bufs.nbytes(c2) != n * 64 or bufs.nbytes(c3) != n * 128:
        raise ValueError("c1, c2, c3 must hold n GT, G1 and G2 elements")
    c2, c3 = bufs.view(c2, n, 1, 64), bufs.view(c3, n, 1, 128)
    d1, d2 = _plan.per_item(d1, n, 1, 128, c2, "d1"), _plan.per_item(d2, n, 1, 64, c2, "d2")
    if not n:
        return bufs.view(c1, 0, 384)
    neg_c2 = bufs.view(engine.g1_sub(bufs.zeros((n * 64,), c2), bufs.flat(c2)), n, 1, 64)
    P = bufs.flat(bufs.cat([d2, neg_c2], 1))                                     # [n, 2, 64]: (d2, -c2)
    Q = bufs.flat(bufs.cat([c3, d1], 1))                                         # [n, 2, 128]: (c3, d1)
    pairs = engine.multi_pair(P, Q, _plan.segments(n, 2))
    return bufs.view(engine.gt_mul(bufs.flat(c1), bufs.flat(pairs)), n, 384)
