"""Host-side planner for batched ZSS04 signatures (Zhang, Safavi-Naini, Susilo 2004): ParamsGenerate
(signature/zss04_signature/zss04_signature.go:129-147), KeyGenerate (:178-193), Sign (:240-257) and Verify (:318-342) for many
signatures at once, and the batch verification the reference does not have.

What is computed, with x the private key, P = [x] g2 the public key and h = H(m) in Zr:

    ParamsGenerate   eG1G2 = e(g1, g2)
    KeyGenerate      P = [x] g2
    Sign             S = [1 / (h + x)] g1
    Verify           e(S, [h] g2 + P) == eG1G2

H is hash.BytesToField (hash/hash_to.go:79-84): fr.SetBytes of the RAW message — the bytes as one big-endian integer modulo r — and
NOT a SHA-256 of it, whatever the reference's comments say.  A message of at most 64 bytes is left-padded with zeros to 64 and reduced
by engine.fr_set_bytes64 (all such messages of a batch in one call); a longer one is reduced on the host.  Ready-made scalar rows
(`hm`) are accepted in place of the messages everywhere.  h + x = 0 mod r makes fr.Element.Inverse return 0 and the signature the point
at infinity, as in the reference; verify_each rejects that signature (e(infinity, .) = 1, which is not eG1G2).

verify_each is the reference's Verify per signature with the same operations in the same order — g2_scalar_mul_base, g2_add,
pair_batch, gt_equal against eG1G2 — and is the DEFINITION of the verdict; the key may be one for the batch or one per signature.

verify_batch takes ONE public key.  The signatures are cut into groups of `group` (the last one short), and with weights rho_i every
group is checked by

    e(sum rho_i h_i S_i - [sum rho_i] g1, g2) . e(sum rho_i S_i, P) == 1

which is the product of the n equations e(S_i, [h_i] g2 + P)^rho_i = eG1G2^rho_i with the pairings of one group folded by bilinearity:
one fr_mul (rho_i h_i), two g1_multi_scalar_mul over the groups, fr_sum_segments for sum rho_i, one g1_scalar_mul_base, one g1_sub, ONE
multi_pair_fixed_q with the two shared points (g2, P) — their lines computed once — and gt_equal against one.  Every signature of a
passing group is accepted; the signatures of the failing groups are gathered by one read of the group verdicts and go through
verify_each.  The result is a verdict per signature and equals verify_each's, except with probability about n / r over the weights.

WHY WEIGHTS.  Without them (all rho_i = 1) the group equation only sees sums: take two valid signatures S_1, S_2 on the SAME message
and replace them with S_1 + D and S_2 - D for any point D.  Each is invalid, the two sums above are unchanged, and the group passes.
Random weights unknown to the forger make the changes rho_1 D - rho_2 D cancel only with probability 1 / r.  rho is an
rng.Randomness — ONE draw of n scalars, one stream, weight i from index i — or n caller-supplied scalar rows, which must be non-zero
modulo r (checked for host rows; a tensor's rows are the caller's promise).  The weights must not be known to whoever made the
signatures.

Out of scope: a key per signature in verify_batch, 128-bit weights, more than one device.

Host orchestration only, engine-agnostic (every function takes the engine: `bn254`, or a stand-in with the same names).  Host arrays
in give host arrays out; CUDA tensors in give CUDA tensors out."""
import numpy as np

from . import _buffers as bufs, _plan
from ._buffers import R_ORDER


def public_params(engine):
    """eG1G2 [384] = e(g1, g2) (ParamsGenerate), a host array"""
    g1, g2 = engine.generators()
    return bufs.view(engine.pair_batch(g1, g2), 384)


def message_scalars(engine, messages, like=None):
    """h [n, 32] = hash.BytesToField(m) for a list of byte strings, of the kind of `like` (host without it): messages of at most 64
    bytes in one fr_set_bytes64, longer ones reduced on the host"""
    msgs = [bytes(m) for m in messages]
    n = len(msgs)
    out = np.zeros((n, 32), dtype=np.uint8)
    short = [i for i, m in enumerate(msgs) if len(m) <= 64]
    for i, m in enumerate(msgs):
        if len(m) > 64:
            out[i] = np.frombuffer((int.from_bytes(m, "big") % R_ORDER).to_bytes(32, "little"), dtype=np.uint8)
    out = out if like is None else bufs.put(out, like)
    if short:
        padded = np.frombuffer(b"".join(msgs[i].rjust(64, b"\0") for i in short), dtype=np.uint8).copy()
        h = bufs.view(engine.fr_set_bytes64(padded if like is None else bufs.put(padded, like)), len(short), 32)
        if len(short) == n:
            return h
        out[bufs.put(np.asarray(short, dtype=np.int64), out)] = h
    return out


def _hm(engine, messages, hm, like, n=None):
    if (messages is None) == (hm is None):
        raise ValueError("give the messages or their scalars (hm), one of the two")
    h = message_scalars(engine, messages, like) if hm is None else _plan.scalars(hm, like)
    if bufs.nbytes(h) % 32 or (n is not None and bufs.nbytes(h) != 32 * n):
        raise ValueError("hm must hold one 32-byte scalar per signature")
    return bufs.view(h, -1, 32)


def keygen_batch(engine, x):
    """P [n, 128] = [x] g2 for n private keys (scalar rows or Python integers)"""
    x = x if _plan.is_buffer(x) else _plan.scalar_rows(x)
    n = bufs.nbytes(x) // 32
    return bufs.view(engine.g2_scalar_mul_base(bufs.flat(x)), n, 128) if n else bufs.empty((0, 128), x)


def sign_batch(engine, x, messages=None, hm=None):
    """S [n, 64] = [1 / (h_i + x)] g1: fr_add, fr_inverse, g1_scalar_mul_base.  x: one private key for the batch or one per message.
    h_i + x = 0 gives the point at infinity."""
    like = hm if _plan.is_buffer(hm) else x if _plan.is_buffer(x) else None
    h = _hm(engine, messages, hm, like if like is not None else np.zeros(0, np.uint8))
    n = h.shape[0]
    if not n:
        return bufs.empty((0, 64), h)
    x = _plan.scalars(x, h)
    if bufs.nbytes(x) not in (32, 32 * n):
        raise ValueError("x must hold one scalar, or one per message")
    x = bufs.flat(bufs.expand(bufs.view(x, -1, 32), n, 32)) if bufs.nbytes(x) == 32 else bufs.flat(x)
    return bufs.view(engine.g1_scalar_mul_base(engine.fr_inverse(engine.fr_add(bufs.flat(h), x))), n, 64)


def verify_each(engine, P, eG1G2, sigs, messages=None, hm=None):
    """ok [n] (uint8): the reference's Verify per signature.  P: one public key ([128]) or one per signature ([n, 128])."""
    n = bufs.nbytes(sigs) // 64
    if bufs.nbytes(sigs) != 64 * n:
        raise ValueError("signatures are G1 points, rows of 64 bytes")
    h = _hm(engine, messages, hm, sigs, n)
    if not n:
        return bufs.empty((0,), sigs)
    P = _plan.public(P, 1 if bufs.nbytes(P) == 128 else n, 128, sigs, "P")
    eg = _plan.public(eG1G2, 1, 384, sigs, "eG1G2")
    q = engine.g2_add(engine.g2_scalar_mul_base(bufs.flat(h)), bufs.flat(P))
    return bufs.view(engine.gt_equal(engine.pair_batch(bufs.flat(sigs), bufs.flat(q)), bufs.flat(eg)), n)


def group_values(engine, P, sigs, h, rho, seg):
    """the left side of the group equation, [groups, 384]: one when the group's weighted equations hold"""
    g1, g2 = engine.generators()
    S = bufs.flat(sigs)
    a = engine.g1_multi_scalar_mul(S, engine.fr_mul(rho, bufs.flat(h)), seg)
    b = engine.g1_multi_scalar_mul(S, rho, seg)
    a = engine.g1_sub(bufs.flat(a), engine.g1_scalar_mul_base(bufs.flat(engine.fr_sum_segments(rho, seg))))
    Q = bufs.cat([_plan.public(g2, 1, 128, sigs, "g2"), bufs.view(P, 1, 128)])
    return engine.multi_pair_fixed_q(_plan.interleave([a, b], 64), bufs.flat(Q))


def verify_batch(engine, P, eG1G2, sigs, rho, messages=None, hm=None, group=1024):
    """ok [n] (uint8) for n signatures under ONE public key P: the group equation of the module text with the weights rho, then
    verify_each on the signatures of the groups that fail.  An all-valid batch makes no pair_batch call."""
    n = bufs.nbytes(sigs) // 64
    if bufs.nbytes(sigs) != 64 * n:
        raise ValueError("signatures are G1 points, rows of 64 bytes")
    seg = _plan.group_table(n, group)
    h = _hm(engine, messages, hm, sigs, n)
    if not n:
        return bufs.empty((0,), sigs)
    P = _plan.public(P, 1, 128, sigs, "P")
    sigs = bufs.view(sigs, n, 64)
    rho = _plan.weights(rho, sigs, n)
    one = _plan.public(_plan.GT_ONE, 1, 384, sigs, "one")
    ok = engine.gt_equal(group_values(engine, P, sigs, h, rho, seg), bufs.flat(one))
    return _plan.settle(ok, n, group, sigs, lambda idx: verify_each(engine, P, eG1G2, bufs.take(sigs, idx), hm=bufs.take(h, idx)))
