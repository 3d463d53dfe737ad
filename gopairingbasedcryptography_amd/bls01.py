"""Host-side planner for batched BLS signatures (Boneh, Lynn, Shacham 2001) as the reference has them, public keys in G1 and
signatures in G2: ParamsGenerate (signature/bls01_signature/bls_signature.go:31-36), KeyGenerate (:38-56), Sign (:58-69) and Verify
(:71-89) for many signatures at once, and the batch verification the reference does not have.

What is computed, with x the private key, X = [x] g1 the public key and H(m) = hash.BytesToG2(m) — bn254.HashToG2 with the tag
hash_to.DST_BYTES_G2:

    KeyGenerate   X = [x] g1
    Sign          sigma = [x] H(m)
    Verify        e(X, H(m)) . e(g1, -sigma) == 1          (bn254.PairingCheck of the two pairs)

verify_each is the reference's Verify per signature with the same operations in the same order — hash_to_g2, the negation of sigma
(g2_sub from the point at infinity), the two-pair product by multi_pair on segments of two, gt_equal against one, which is what
PairingCheck tests — and is the DEFINITION of the verdict; the key may be one for the batch or one per signature.  The point at infinity
as a signature is rejected (e(X, H) alone is not one).  Ready-made points H (`hashed`) are accepted in place of the messages.

verify_batch takes ONE public key.  The signatures are cut into groups of `group` (the last one short), and with weights rho_i every
group is checked by

    e(X, sum rho_i H_i) . e(-g1, sum rho_i sigma_i) == 1

the product of the n equations raised to rho_i with the pairings of one group folded by bilinearity: two g2_multi_scalar_mul over the
groups, multi_pair on two-pair segments and gt_equal against one.  Every signature of a passing group is accepted; the signatures of
the failing groups are gathered by one read of the group verdicts and go through verify_each.  The result is a verdict per signature and
equals verify_each's, except with probability about n / r over the weights — and under ONE PRESUMPTION: the batch form needs sigma_i
and H_i in the subgroup of order r of the twist (G2), because only there does a weight act modulo r.  The curve E'(Fp2) has a cofactor;
a "signature" with a component outside G2 could be weighted away for a weight divisible by that component's small order.  g2_unmarshal
(gnark's subgroup check) and hash_to_g2 (cofactor clearing) guarantee membership for whatever they return, so signatures that came in
through them are fine; verify_each makes no such assumption, and neither does gnark's PairingCheck.

WHY WEIGHTS.  With all rho_i = 1 the equation only sees sums: two valid signatures sigma_1, sigma_2 (on any messages), replaced by
sigma_1 + D and sigma_2 - D, are both invalid and leave sum sigma_i unchanged, so the group passes.  rho is an rng.Randomness (ONE draw
of n scalars, one stream, weight i from index i) or n caller-supplied scalar rows, non-zero modulo r (checked for host rows; a tensor's
rows are the caller's promise), unknown to whoever made the signatures.

Out of scope: a key per signature in verify_batch (distinct keys need a pairing per key), 128-bit weights, more than one device.

Host orchestration only, engine-agnostic.  Host arrays in give host arrays out; CUDA tensors in give CUDA tensors out."""
import numpy as np

from . import _buffers as bufs, _plan

DST_BYTES_G2 = b"Hash Bytes To Element In G2"            # hash_to.DST_BYTES_G2, the tag of hash.BytesToG2


def public_params(engine):
    """g1 [64] (ParamsGenerate), a host array"""
    return bufs.view(engine.generators()[0], 64)


def keygen_batch(engine, x):
    """X [n, 64] = [x] g1 for n private keys (scalar rows or Python integers)"""
    x = x if _plan.is_buffer(x) else _plan.scalar_rows(x)
    n = bufs.nbytes(x) // 32
    return bufs.view(engine.g1_scalar_mul_base(bufs.flat(x)), n, 64) if n else bufs.empty((0, 64), x)


def hash_messages(engine, messages, msg_off=None):
    """H [n, 128] = hash.BytesToG2(m): a list of byte strings, or a flat buffer with msg_off as hash_to_g2 takes them (host or CUDA)"""
    if msg_off is None and not _plan.is_buffer(messages):
        messages = [bytes(m) for m in messages]
        if not messages:
            return np.zeros((0, 128), dtype=np.uint8)
    h = engine.hash_to_g2(messages, DST_BYTES_G2, msg_off)
    return bufs.view(h, bufs.nbytes(h) // 128, 128)


def _hashed(engine, messages, hashed, like=None):
    if (messages is None) == (hashed is None):
        raise ValueError("give the messages or their points (hashed), one of the two")
    h = hash_messages(engine, messages) if hashed is None else hashed
    if bufs.nbytes(h) % 128:
        raise ValueError("hashed holds G2 points, rows of 128 bytes")
    h = bufs.view(h, bufs.nbytes(h) // 128, 128)
    return bufs.put(h, like) if like is not None and not bufs.is_torch(h) else h


def sign_batch(engine, x, messages=None, hashed=None):
    """sigma [n, 128] = [x] H(m_i): one g2_scalar_mul.  x: one private key for the batch or one per message."""
    h = _hashed(engine, messages, hashed, x if bufs.is_torch(x) else None)
    n = h.shape[0]
    if not n:
        return bufs.empty((0, 128), h)
    x = _plan.scalars(x, h)
    if bufs.nbytes(x) not in (32, 32 * n):
        raise ValueError("x must hold one scalar, or one per message")
    x = bufs.flat(bufs.expand(bufs.view(x, -1, 32), n, 32)) if bufs.nbytes(x) == 32 else bufs.flat(x)
    return bufs.view(engine.g2_scalar_mul(bufs.flat(h), x), n, 128)


def _sigs(sigs):
    n = bufs.nbytes(sigs) // 128
    if bufs.nbytes(sigs) != 128 * n:
        raise ValueError("signatures are G2 points, rows of 128 bytes")
    return n, bufs.view(sigs, n, 128)


def verify_each(engine, X, g1, sigs, messages=None, hashed=None):
    """ok [n] (uint8): the reference's Verify per signature.  X: one public key ([64]) or one per signature ([n, 64])."""
    n, sigs = _sigs(sigs)
    h = _hashed(engine, messages, hashed, sigs)
    if h.shape[0] != n:
        raise ValueError("%d messages for %d signatures" % (h.shape[0], n))
    if not n:
        return bufs.empty((0,), sigs)
    X = _plan.per_item(X, n, 1, 64, sigs, "X")
    g = bufs.expand(_plan.public(g1, 1, 64, sigs, "g1"), n, 64)
    neg = engine.g2_sub(bufs.flat(bufs.zeros((n, 128), sigs)), bufs.flat(sigs))
    prod = engine.multi_pair(_plan.interleave([X, g], 64), _plan.interleave([h, neg], 128), _plan.segments(n, 2))
    return bufs.view(engine.gt_equal(prod, bufs.flat(_plan.public(_plan.GT_ONE, 1, 384, sigs, "one"))), n)


def group_values(engine, X, g1, sigs, h, rho, seg):
    """the left side of the group equation, [groups, 384]: one when the group's weighted equations hold"""
    a = engine.g2_multi_scalar_mul(bufs.flat(h), rho, seg)
    b = engine.g2_multi_scalar_mul(bufs.flat(sigs), rho, seg)
    groups = len(seg) - 1
    neg_g1 = _plan.public(engine.g1_neg(np.asarray(g1.cpu() if bufs.is_torch(g1) else g1, dtype=np.uint8).reshape(64)), 1, 64, sigs, "g1")
    P = _plan.interleave([bufs.expand(X, groups, 64), bufs.expand(neg_g1, groups, 64)], 64)
    return engine.multi_pair(P, _plan.interleave([a, b], 128), _plan.segments(groups, 2))


def verify_batch(engine, X, g1, sigs, rho, messages=None, hashed=None, group=1024):
    """ok [n] (uint8) for n signatures under ONE public key X: the group equation of the module text with the weights rho, then
    verify_each on the signatures of the groups that fail."""
    n, sigs = _sigs(sigs)
    seg = _plan.group_table(n, group)
    h = _hashed(engine, messages, hashed, sigs)
    if h.shape[0] != n:
        raise ValueError("%d messages for %d signatures" % (h.shape[0], n))
    if not n:
        return bufs.empty((0,), sigs)
    X = _plan.public(X, 1, 64, sigs, "X")
    rho = _plan.weights(rho, sigs, n)
    one = _plan.public(_plan.GT_ONE, 1, 384, sigs, "one")
    ok = engine.gt_equal(group_values(engine, X, g1, sigs, h, rho, seg), bufs.flat(one))
    return _plan.settle(ok, n, group, sigs, lambda idx: verify_each(engine, X, g1, bufs.take(sigs, idx), hashed=bufs.take(h, idx)))
