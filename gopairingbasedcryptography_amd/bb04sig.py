"""Host-side planner for batched BB04 signatures (Boneh, Boyen 2004, the full scheme): ParamsGenerate
(signature/bb04_signature/bb04_signature.go:134-147), KeyGenerate (:171-190), Sign (:221-240) and Verify (:273-297) for many signatures
at once, and the batch verification the reference does not have.

What is computed, with (alpha, beta) the private key, Y = [alpha] g2 and Z = [beta] g2 the public key, m in Zr the message and r in Zr
the signature's randomness:

    ParamsGenerate   eG1G2 = e(g1, g2)
    KeyGenerate      Y = [alpha] g2        Z = [beta] g2
    Sign             sigma = [1 / (alpha + r beta + m)] g1        the signature is (r, sigma)
    Verify           e(sigma, Y + ([r] Z + [m] g2)) == eG1G2

The message IS a scalar (Message.MessageFr): there is no hash.  alpha + r beta + m = 0 mod r makes fr.Element.Inverse return 0 and
sigma the point at infinity, as in the reference; verify_each rejects it.  sign_batch takes r as an argument; sign_batch_seeded draws it
on the device: ONE draw of an rng.Randomness, r [n], one stream, r_i from index i.

verify_each is the reference's Verify per signature with the same operations in the same order — g2_scalar_mul, g2_scalar_mul_base,
g2_add twice, pair_batch, gt_equal against eG1G2 — and is the DEFINITION of the verdict; the key may be one for the batch or one per
signature.

verify_batch takes ONE public key.  The signatures are cut into groups of `group` (the last one short), and with weights rho_i every
group is checked by

    e(sum rho_i sigma_i, Y) . e(sum rho_i r_i sigma_i, Z) . e(sum rho_i m_i sigma_i - [sum rho_i] g1, g2) == 1

the product of the n equations raised to rho_i with the pairings of one group folded by bilinearity: two fr_mul, three
g1_multi_scalar_mul over the groups, fr_sum_segments, one g1_scalar_mul_base, one g1_sub, ONE multi_pair_fixed_q with the three shared
points (Y, Z, g2) and gt_equal against one.  Every signature of a passing group is accepted; the signatures of the failing groups are
gathered by one read of the group verdicts and go through verify_each.  The result is a verdict per signature and equals verify_each's,
except with probability about n / r over the weights.

WHY WEIGHTS.  With all rho_i = 1 the equation only sees sums: two valid signatures (r, sigma_1), (r, sigma_2) on the same message with
the same r, replaced by sigma_1 + D and sigma_2 - D, are both invalid and leave every sum unchanged.  rho is an rng.Randomness (ONE
draw of n scalars, one stream, weight i from index i) or n caller-supplied scalar rows, non-zero modulo r (checked for host rows; a
tensor's rows are the caller's promise), unknown to whoever made the signatures.

Out of scope: a key per signature in verify_batch, 128-bit weights, more than one device.

Host orchestration only, engine-agnostic.  Host arrays in give host arrays out; CUDA tensors in give CUDA tensors out."""
from . import _buffers as bufs, _plan


def public_params(engine):
    """eG1G2 [384] = e(g1, g2) (ParamsGenerate), a host array"""
    g1, g2 = engine.generators()
    return bufs.view(engine.pair_batch(g1, g2), 384)


def keygen_batch(engine, alpha, beta):
    """(Y [n, 128], Z [n, 128]) = ([alpha] g2, [beta] g2) for n private keys (scalar rows or Python integers)"""
    alpha = alpha if _plan.is_buffer(alpha) else _plan.scalar_rows(alpha)
    n = bufs.nbytes(alpha) // 32
    beta = _plan.scalars(beta, alpha, n, "beta")
    if not n:
        return bufs.empty((0, 128), alpha), bufs.empty((0, 128), alpha)
    return bufs.view(engine.g2_scalar_mul_base(bufs.flat(alpha)), n, 128), bufs.view(engine.g2_scalar_mul_base(beta), n, 128)


def _key_scalars(v, like, n, what):
    v = _plan.scalars(v, like)
    if bufs.nbytes(v) not in (32, 32 * n):
        raise ValueError("%s must hold one scalar, or one per message" % what)
    return bufs.flat(bufs.expand(bufs.view(v, -1, 32), n, 32)) if bufs.nbytes(v) == 32 else bufs.flat(v)


def sign_batch(engine, alpha, beta, m, r):
    """(r [n, 32], sigma [n, 64]) with sigma_i = [1 / (alpha + r_i beta + m_i)] g1: fr_mul, fr_add twice in the reference's order,
    fr_inverse, g1_scalar_mul_base.  alpha, beta: one private key for the batch or one per message; m, r: n scalars."""
    like = next((v for v in (m, r, alpha) if _plan.is_buffer(v)), None)
    m = m if _plan.is_buffer(m) else _plan.scalars(m, like if like is not None else _plan.scalar_rows([]))
    n = bufs.nbytes(m) // 32
    r = _plan.scalars(r, m, n, "r")
    if not n:
        return bufs.empty((0, 32), m), bufs.empty((0, 64), m)
    alpha, beta = _key_scalars(alpha, m, n, "alpha"), _key_scalars(beta, m, n, "beta")
    d = engine.fr_add(engine.fr_add(alpha, engine.fr_mul(r, beta)), bufs.flat(m))
    return bufs.view(r, n, 32), bufs.view(engine.g1_scalar_mul_base(engine.fr_inverse(d)), n, 64)


def sign_batch_seeded(engine, alpha, beta, m, rng):
    """sign_batch with r drawn on the device: ONE draw of rng (an rng.Randomness over the engine), r [n], so the signatures are
    reproducible from the seed.  The seed is key material."""
    m = m if _plan.is_buffer(m) else _plan.scalar_rows(m)
    return sign_batch(engine, alpha, beta, m, rng.scalars(m, bufs.nbytes(m) // 32))


def _sig(r, sigma):
    n = bufs.nbytes(sigma) // 64
    if bufs.nbytes(sigma) != 64 * n:
        raise ValueError("sigma holds G1 points, rows of 64 bytes")
    return n, _plan.scalars(r, sigma, n, "r")


def verify_each(engine, Y, Z, eG1G2, m, r, sigma):
    """ok [n] (uint8): the reference's Verify per signature.  Y, Z: one public key ([128] each) or one per signature ([n, 128])."""
    n, r = _sig(r, sigma)
    m = _plan.scalars(m, sigma, n, "m")
    if not n:
        return bufs.empty((0,), sigma)
    Y = _plan.public(Y, 1 if bufs.nbytes(Y) == 128 else n, 128, sigma, "Y")
    Z = _plan.public(Z, 1 if bufs.nbytes(Z) == 128 else n, 128, sigma, "Z")
    eg = _plan.public(eG1G2, 1, 384, sigma, "eG1G2")
    t = engine.g2_add(engine.g2_scalar_mul(bufs.flat(Z), r), engine.g2_scalar_mul_base(m))
    q = engine.g2_add(bufs.flat(bufs.expand(Y, n, 128)) if Y.shape[0] == 1 else bufs.flat(Y), t)
    return bufs.view(engine.gt_equal(engine.pair_batch(bufs.flat(sigma), bufs.flat(q)), bufs.flat(eg)), n)


def group_values(engine, Y, Z, m, r, sigma, rho, seg):
    """the left side of the group equation, [groups, 384]: one when the group's weighted equations hold"""
    g1, g2 = engine.generators()
    S = bufs.flat(sigma)
    a = engine.g1_multi_scalar_mul(S, rho, seg)
    b = engine.g1_multi_scalar_mul(S, engine.fr_mul(rho, r), seg)
    c = engine.g1_multi_scalar_mul(S, engine.fr_mul(rho, m), seg)
    c = engine.g1_sub(bufs.flat(c), engine.g1_scalar_mul_base(bufs.flat(engine.fr_sum_segments(rho, seg))))
    Q = bufs.cat([bufs.view(Y, 1, 128), bufs.view(Z, 1, 128), _plan.public(g2, 1, 128, sigma, "g2")])
    return engine.multi_pair_fixed_q(_plan.interleave([a, b, c], 64), bufs.flat(Q))


def verify_batch(engine, Y, Z, eG1G2, m, r, sigma, rho, group=1024):
    """ok [n] (uint8) for n signatures under ONE public key (Y, Z): the group equation of the module text with the weights rho, then
    verify_each on the signatures of the groups that fail.  An all-valid batch makes no pair_batch call."""
    n, r = _sig(r, sigma)
    seg = _plan.group_table(n, group)
    m = _plan.scalars(m, sigma, n, "m")
    if not n:
        return bufs.empty((0,), sigma)
    Y, Z = _plan.public(Y, 1, 128, sigma, "Y"), _plan.public(Z, 1, 128, sigma, "Z")
    sigma = bufs.view(sigma, n, 64)
    rho = _plan.weights(rho, sigma, n)
    one = _plan.public(_plan.GT_ONE, 1, 384, sigma, "one")
    ok = engine.gt_equal(group_values(engine, Y, Z, m, r, sigma, rho, seg), bufs.flat(one))
    m2, r2 = bufs.view(m, n, 32), bufs.view(r, n, 32)
    return _plan.settle(ok, n, group, sigma, lambda idx: verify_each(engine, Y, Z, eG1G2, bufs.flat(bufs.take(m2, idx)), bufs.flat(bufs.take(r2, idx)), bufs.take(sigma, idx)))
