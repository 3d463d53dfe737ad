"""Host-side planner for batched ASBB, the aggregatable signature-based broadcast of Wu, Mu, Susilo, Qin and Domingo-Ferrer's asymmetric
group key agreement (EUROCRYPT 2009) as the reference has it (gka/agka09/asbb.go): KeyGen (:82-113), Sign (:115-121), Verify (:123-146),
Encrypt (:148-171), Decrypt (:173-191), AggregatePublicKeys (:193-207) and AggregateSignatures (:209-220) for many items at once, the
batch verification the reference does not have, and the validation of contributed elements it does not have either.

What is computed, with the private key (r, X), the public key (R, A) and H(s) = hash.BytesToG1(s) — bn254.HashToG1 with the tag
hash_to.DST_BYTES_G1:

    KeyGen       X = [x] g1,  R = [-r] g2,  A = e(X, g2)
    Sign         sigma = X + [r] H(s)
    Verify       e(sigma, g2) . e(H(s), R) == A
    Encrypt      c1 = [t] g2,  c2 = [t] R,  c3 = m . A^t
    Decrypt      m = c3 / (e(sigma, c1) . e(H(s), c2))
    Aggregate    R = sum R_i,  A = prod A_i,  sigma = sum sigma_i

Key homomorphism (asbb.go:21-30): the signatures of several members on ONE string add up to a signature under the aggregated key, which
also decrypts what was encrypted under that key.  Every result is bit-equal to the reference's: the same group operations on the same
operands, and the engine's outputs are canonical.

verify_each is the reference's Verify per signature, the pairs in its order — (sigma, g2) then (H(s), R), one two-pair multi_pair segment
per item, gt_equal against A — and is the DEFINITION of the verdict; the key may be one for the batch or one per signature.

verify_batch takes ONE public key.  The signatures are cut into groups of `group` (the last one short), and with weights rho_i every
group is checked by

    e(sum rho_i sigma_i, g2) . e(sum rho_i H_i, R) == A^(sum rho_i)

the product of the n equations raised to rho_i with the pairings of one group folded by bilinearity: two g1_multi_scalar_mul over the
groups, fr_sum_segments, ONE multi_pair_fixed_q with the two shared points (g2, R), gt_exp and gt_equal.  Every signature of a passing
group is accepted; the signatures of the failing groups are gathered by one read of the group verdicts and go through verify_each.  The
weight rules are ZSS04's (zss04.py, WHY WEIGHTS): without weights S + D and S - D on one string pass together; rho is an rng.Randomness
(ONE draw of n scalars) or n caller-supplied rows, non-zero modulo r, unknown to whoever made the signatures.  G1 has cofactor 1, so a
signature on the curve is in the group and a weight acts on it modulo r; a signature off the curve is the caller's to reject
(validate=True in verify_each, bn254.g1_is_on_curve).

VALIDATION.  ASBB is the scheme of the reference in which elements contributed by OTHER parties are aggregated: a public key is
(R in G2, A in GT) from another member.  With validate=True aggregate_public_keys tests every R by g2_is_in_subgroup and every A by
gt_is_in_subgroup, aggregate_signatures every sigma by g1_is_on_curve; a rejected element is replaced by the neutral element BEFORE the
sums and products, so it enters none; the per-element mask comes back beside the results, and a group with a rejected element gives an
all-zero row and ok = 0 — the convention of the unmarshal entries.  An element of the wrong order in an unchecked sum is what these
tests are for: R off the subgroup, or A in the cyclotomic subgroup but not of order r.

Out of scope: validation inside decrypt_batch, verify_batch over distinct keys, a segment table in device memory, more than one
device, the group-key-agreement protocol around ASBB.

Host orchestration only, engine-agnostic (every function takes the engine: `bn254`, or a stand-in with the same names).  Host arrays
in give host arrays out; CUDA tensors in give CUDA tensors out."""
import numpy as np

from . import _buffers as bufs, _plan

DST_BYTES_G1 = b"Hash Bytes To Element In G1"            # hash_to.DST_BYTES_G1, the tag of hash.BytesToG1


def public_params(engine):
    """(g1 [64], g2 [128]) (ParaGen), host arrays"""
    g1, g2 = engine.generators()
    return bufs.view(g1, 64), bufs.view(g2, 128)


def keygen_batch(engine, r, x):
    """(R [n, 128], A [n, 384], X [n, 64]) for n private scalars r and x (scalar rows or Python integers): X = [x] g1 by
    g1_scalar_mul_base, R = [-r] g2 by fr_neg and g2_scalar_mul_base, A = e(X, g2) by pair_batch.  (r, X) is the private key."""
    x = x if _plan.is_buffer(x) else _plan.scalar_rows(x)
    r = _plan.scalars(r, x)
    n = bufs.nbytes(x) // 32
    if bufs.nbytes(r) != 32 * n or bufs.is_torch(r) != bufs.is_torch(x):
        raise ValueError("r and x must hold one scalar per key, of one kind")
    if not n:
        return bufs.empty((0, 128), x), bufs.empty((0, 384), x), bufs.empty((0, 64), x)
    X = bufs.view(engine.g1_scalar_mul_base(bufs.flat(x)), n, 64)
    R = bufs.view(engine.g2_scalar_mul_base(bufs.flat(engine.fr_neg(bufs.flat(r)))), n, 128)
    g2 = bufs.expand(_plan.public(engine.generators()[1], 1, 128, X, "g2"), n, 128)
    return R, bufs.view(engine.pair_batch(bufs.flat(X), bufs.flat(g2)), n, 384), X


def hash_strings(engine, strings, msg_off=None):
    """H [n, 64] = hash.BytesToG1(s): a list of byte strings, or a flat buffer with msg_off as hash_to_g1 takes them (host or CUDA)"""
    if msg_off is None and not _plan.is_buffer(strings):
        strings = [bytes(s) for s in strings]
        if not strings:
            return np.zeros((0, 64), dtype=np.uint8)
    h = engine.hash_to_g1(strings, DST_BYTES_G1, msg_off)
    return bufs.view(h, bufs.nbytes(h) // 64, 64)


def _hashed(engine, strings, hashed, like=None):
    if (strings is None) == (hashed is None):
        raise ValueError("give the strings or their points (hashed), one of the two")
    h = hash_strings(engine, strings) if hashed is None else hashed
    if bufs.nbytes(h) % 64:
        raise ValueError("hashed holds G1 points, rows of 64 bytes")
    h = bufs.view(h, bufs.nbytes(h) // 64, 64)
    return bufs.put(h, like) if like is not None and not bufs.is_torch(h) else h


def _points(x, width, what):
    n = bufs.nbytes(x) // width
    if bufs.nbytes(x) != width * n:
        raise ValueError("%s: rows of %d bytes" % (what, width))
    return n, bufs.view(x, n, width)


def sign_batch(engine, r, X, strings=None, hashed=None):
    """sigma [n, 64] = X + [r] H(s_i): g1_scalar_mul, g1_add.  (r, X): one private key for the batch, or one per item."""
    like = X if bufs.is_torch(X) else r if bufs.is_torch(r) else None
    h = _hashed(engine, strings, hashed, like)
    n = h.shape[0]
    if not n:
        return bufs.empty((0, 64), h)
    r = _plan.scalars(r, h)
    if bufs.nbytes(r) not in (32, 32 * n):
        raise ValueError("r must hold one scalar, or one per item")
    r = bufs.flat(bufs.expand(bufs.view(r, -1, 32), n, 32)) if bufs.nbytes(r) == 32 else bufs.flat(r)
    X = _plan.per_item(X, n, 1, 64, h, "X")
    return bufs.view(engine.g1_add(bufs.flat(X), engine.g1_scalar_mul(bufs.flat(h), r)), n, 64)


def _two_pairs(engine, first_g1, h, first_g2, second_g2, n):
    """e(first_g1[i], first_g2[i]) . e(h[i], second_g2[i]) per item, [n * 384]: one two-pair segment each, the pairs in this order"""
    return engine.multi_pair(_plan.interleave([first_g1, h], 64), _plan.interleave([first_g2, second_g2], 128), _plan.segments(n, 2))


def _and(a, b):
    return bufs.view(a, -1) & bufs.view(b, -1)


def _only(mask, rows, width, neutral=None):
    """rows [n, width] with the rows of mask = 0 replaced by the neutral element (all zero: the point at infinity)"""
    m = bufs.view(mask, -1, 1)
    kept = bufs.view(rows, -1, width) * m
    return kept if neutral is None else kept + bufs.view(neutral, 1, width) * (1 - m)


def verify_each(engine, R, A, sigs, strings=None, hashed=None, validate=False):
    """ok [n] (uint8): the reference's Verify per signature.  (R, A): one public key ([128], [384]) or one per signature.
    validate=True: a signature that is not on the curve (g1_is_on_curve) gets the verdict 0 and enters the pairing as infinity."""
    n, sigs = _points(sigs, 64, "signatures are G1 points")
    h = _hashed(engine, strings, hashed, sigs)
    if h.shape[0] != n:
        raise ValueError("%d strings for %d signatures" % (h.shape[0], n))
    if not n:
        return bufs.empty((0,), sigs)
    R = _plan.per_item(R, n, 1, 128, sigs, "R")
    A = _plan.public(A, 1 if bufs.nbytes(A) == 384 else n, 384, sigs, "A")
    g2 = bufs.expand(_plan.public(engine.generators()[1], 1, 128, sigs, "g2"), n, 128)
    on = None
    if validate:
        on = bufs.view(engine.g1_is_on_curve(bufs.flat(sigs)), n)
        sigs = _only(on, sigs, 64)
    ok = bufs.view(engine.gt_equal(_two_pairs(engine, sigs, h, g2, R, n), bufs.flat(A)), n)
    return ok if on is None else _and(ok, on)


def group_values(engine, R, sigs, h, rho, seg):
    """the left side of the group equation, [groups, 384]"""
    a = engine.g1_multi_scalar_mul(bufs.flat(sigs), rho, seg)
    b = engine.g1_multi_scalar_mul(bufs.flat(h), rho, seg)
    Q = bufs.cat([_plan.public(engine.generators()[1], 1, 128, sigs, "g2"), bufs.view(R, 1, 128)])
    return engine.multi_pair_fixed_q(_plan.interleave([a, b], 64), bufs.flat(Q))


def verify_batch(engine, R, A, sigs, rho, strings=None, hashed=None, group=1024):
    """ok [n] (uint8) for n signatures under ONE public key (R, A): the group equation of the module text with the weights rho, then
    verify_each on the signatures of the groups that fail.  An all-valid batch makes no per-item pairing."""
    n, sigs = _points(sigs, 64, "signatures are G1 points")
    seg = _plan.group_table(n, group)
    h = _hashed(engine, strings, hashed, sigs)
    if h.shape[0] != n:
        raise ValueError("%d strings for %d signatures" % (h.shape[0], n))
    if not n:
        return bufs.empty((0,), sigs)
    R, A = _plan.public(R, 1, 128, sigs, "R"), _plan.public(A, 1, 384, sigs, "A")
    rho = _plan.weights(rho, sigs, n)
    groups = len(seg) - 1
    right = engine.gt_exp(bufs.flat(bufs.expand(A, groups, 384)), bufs.flat(engine.fr_sum_segments(rho, seg)))
    ok = engine.gt_equal(group_values(engine, R, sigs, h, rho, seg), bufs.flat(right))
    return _plan.settle(ok, n, group, sigs, lambda idx: verify_each(engine, R, A, bufs.take(sigs, idx), hashed=bufs.take(h, idx)))


def encrypt_batch(engine, R, A, messages, t):
    """(c1 [n, 128], c2 [n, 128], c3 [n, 384]) = ([t] g2, [t] R, m . A^t) for n plaintexts in GT and n scalars t (rows or Python integers):
    g2_scalar_mul_base, g2_scalar_mul, gt_exp, gt_mul.  (R, A): one public key for the batch, or one per plaintext."""
    n, messages = _points(messages, 384, "plaintexts are GT elements")
    if not n:
        return bufs.empty((0, 128), messages), bufs.empty((0, 128), messages), bufs.empty((0, 384), messages)
    t = _plan.scalars(t, messages, n, "t")
    R, A = _plan.per_item(R, n, 1, 128, messages, "R"), _plan.per_item(A, n, 1, 384, messages, "A")
    c1 = bufs.view(engine.g2_scalar_mul_base(t), n, 128)
    c2 = bufs.view(engine.g2_scalar_mul(bufs.flat(R), t), n, 128)
    c3 = bufs.view(engine.gt_mul(bufs.flat(messages), engine.gt_exp(bufs.flat(A), t)), n, 384)
    return c1, c2, c3


def encrypt_batch_seeded(engine, R, A, messages, rng):
    """encrypt_batch with t drawn from `rng` (rng.Randomness): ONE draw of n scalars, t_i from index i"""
    n, messages = _points(messages, 384, "plaintexts are GT elements")
    return encrypt_batch(engine, R, A, messages, rng.scalars(messages, n))


def decrypt_batch(engine, c1, c2, c3, sigs, strings=None, hashed=None):
    """m [n, 384] = c3 / (e(sigma, c1) . e(H(s), c2)): one two-pair multi_pair segment per item and one gt_div.  sigma: one signature
    for the batch ([64], with one string) or one per ciphertext."""
    n, c3 = _points(c3, 384, "c3 holds GT elements")
    if not n:
        return bufs.empty((0, 384), c3)
    c1, c2 = _plan.public(c1, n, 128, c3, "c1"), _plan.public(c2, n, 128, c3, "c2")
    h = _hashed(engine, strings, hashed, c3)
    if h.shape[0] not in (1, n):
        raise ValueError("%d strings for %d ciphertexts" % (h.shape[0], n))
    h = bufs.expand(h, n, 64) if h.shape[0] != n else h
    sigs = bufs.view(_plan.per_item(sigs, n, 1, 64, c3, "sigma"), n, 64)
    return bufs.view(engine.gt_div(bufs.flat(c3), _two_pairs(engine, sigs, h, c1, c2, n)), n, 384)


def _groups(seg_off, n, what):
    """the host table of the groups to aggregate; an empty group is the reference's error"""
    seg = np.ascontiguousarray(seg_off, dtype=np.uint64).reshape(-1)
    if seg.size < 2 or int(seg[0]) != 0 or int(seg[-1]) != n:
        raise ValueError("seg_off must run from 0 to the number of %s, one group at least" % what)
    if (np.diff(seg.astype(np.int64)) <= 0).any():
        raise ValueError("no %s provided: every group must hold one at least" % what)
    return seg


def _group_ok(mask, seg, like):
    """ok [groups] of the kind of `like`: 1 where every element of the group has mask = 1 (ONE read of the mask)"""
    host = mask.cpu().numpy() if bufs.is_torch(mask) else np.asarray(mask)
    return bufs.put(np.minimum.reduceat(host.reshape(-1), seg[:-1].astype(np.int64)).astype(np.uint8), like)


def aggregate_public_keys(engine, R, A, seg_off, validate=False):
    """(R [groups, 128], A [groups, 384]) = (sum R_i, prod A_i) over the keys seg_off[s] .. seg_off[s+1] of every group: g2_sum_segments and
    gt_prod.  An empty group raises ValueError, as the reference returns an error.
    validate=True: (R, A, ok [groups], mask [n]) with mask[i] = 1 where R_i passes g2_is_in_subgroup and A_i passes gt_is_in_subgroup; a
    rejected key enters the sums as (infinity, one); a group that holds one has all-zero rows and ok = 0."""
    n, R = _points(R, 128, "R holds G2 points")
    nA, A = _points(A, 384, "A holds GT elements")
    if nA != n:
        raise ValueError("%d R for %d A" % (n, nA))
    seg = _groups(seg_off, n, "public keys")
    if not validate:
        return bufs.view(engine.g2_sum_segments(bufs.flat(R), seg), -1, 128), bufs.view(engine.gt_prod(bufs.flat(A), seg), -1, 384)
    mask = _and(engine.g2_is_in_subgroup(bufs.flat(R)), engine.gt_is_in_subgroup(bufs.flat(A)))
    one = _plan.public(_plan.GT_ONE, 1, 384, A, "one")
    aR = bufs.view(engine.g2_sum_segments(bufs.flat(_only(mask, R, 128)), seg), -1, 128)
    aA = bufs.view(engine.gt_prod(bufs.flat(_only(mask, A, 384, one)), seg), -1, 384)
    ok = _group_ok(mask, seg, R)
    return _only(ok, aR, 128), _only(ok, aA, 384), ok, mask


def aggregate_signatures(engine, sigma, seg_off, validate=False):
    """sigma [groups, 64] = sum sigma_i over every group: g1_sum_segments.  An empty group raises ValueError.
    validate=True: (sigma, ok [groups], mask [n]) with mask[i] = g1_is_on_curve(sigma_i); a rejected signature enters the sums as
    infinity; a group that holds one has an all-zero row and ok = 0."""
    n, sigma = _points(sigma, 64, "signatures are G1 points")
    seg = _groups(seg_off, n, "signatures")
    if not validate:
        return bufs.view(engine.g1_sum_segments(bufs.flat(sigma), seg), -1, 64)
    mask = bufs.view(engine.g1_is_on_curve(bufs.flat(sigma)), n)
    agg = bufs.view(engine.g1_sum_segments(bufs.flat(_only(mask, sigma, 64)), seg), -1, 64)
    ok = _group_ok(mask, seg, sigma)
    return _only(ok, agg, 64), ok, mask
