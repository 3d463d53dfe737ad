"""Host-side planner for batched Gentry 2006 identity-based encryption: KeyGenerate (ibe/gentry06_ibe/gentry06_ibe.go:145-180), Encrypt
(:192-245) and Decrypt (:264-314) for many identities / messages at once, in both of the reference's packages — k = 3 public points
h_1, h_2, h_3 is the CCA-secure gentry06_ibe, k = 1 is gentry06_cpa_ibe (no y, no check).  k is read from the arguments.

What is computed, with ID and every r, s in Zr:

    KeyGenerate   hid_j = [1 / (alpha - ID)] (h_j + [-r_j] g2),  j = 1 .. k         the key is (r_j, hid_j); ID = alpha has none
    Encrypt       u = [s] g1^alpha + [-s ID] g1     v = e(g1, g2)^s     w = M e(g1, h_1)^(-s)
                  beta = H(u, v, w)                 y = e(g1, h_2)^s e(g1, h_3)^(s beta)
    Decrypt       beta = H(u, v, w)                 y' = v^(r_2 + r_3 beta) e(u, hid_2 + [beta] hid_3)    refuse unless y' = y
                  M = w e(u, hid_1) v^(r_1)

H is fr.SetBytes(SHA-256(u.Bytes() || v.Bytes() || w.Bytes())) (:319-343): engine.hash_g1_gt_gt_to_fr, ONE launch that reads the
elements where the step before left them and writes the scalars the next step takes — in the reference's shape that hash sits between
two pieces of group arithmetic in Encrypt and ahead of everything in Decrypt, so a batch that hashed on the host would stop the stream
there twice.  The check of Decrypt is the reference's code as it stands (its own comment says that it differs from the paper's).
The four pairings e(g1, g2), e(g1, h_j) depend on the public parameters alone: public_pairings computes them once, the reference on
every Encrypt.

Host orchestration only, engine-agnostic (every function takes the engine: `bn254`, or a stand-in with the same names).  The
randomness r / s comes in as arguments (scalar rows, or Python integers).  Host arrays in give host arrays out; CUDA tensors in give
CUDA tensors out, every step takes device rows and leaves device rows, and nothing per item crosses PCIe but what the caller passes
in and takes out (the shared points and pairings, and integer arguments, travel once)."""
import numpy as np

from . import _buffers as bufs, _plan


def _repeat(x, n, rows, width):
    """[rows, width] once per item: [n * rows * width], flat"""
    return bufs.flat(bufs.expand(bufs.view(x, 1, rows, width), n, rows, width))


def _k_of(rows, what):
    if rows not in (1, 3):
        raise ValueError("%s: one point (gentry06_cpa_ibe) or three (gentry06_ibe), got %d" % (what, rows))
    return rows


def keygen_batch(engine, alpha, h, ids, r):
    """(rids [n, k, 32], hids [n, k, 128], ok [n]) for n identities.  alpha: the master key (an integer or one scalar row); h: the k
    public points h_j, [k, 128]; ids: n scalars; r: n x k scalars, the r_j of every identity.  fr_sub and fr_inverse give
    1 / (alpha - ID), fr_neg and g2_scalar_mul_base give [-r_j] g2, g2_add and g2_scalar_mul the key points.  Where alpha - ID = 0 the
    reference returns "your identity is invalid (ID equals alpha)" (:151-154): ok = 0 and both rows of that identity are all zero
    (the inverse of 0 is 0 and [0] P is the point at infinity, so its lanes do no harm); every other identity is unaffected."""
    k = _k_of(bufs.nbytes(h) // 128 if bufs.nbytes(h) % 128 == 0 else 0, "h")
    h = bufs.view(h, k, 128)
    ids = _plan.scalars(ids, h)
    n = bufs.nbytes(ids) // 32
    ids, r, alpha = _plan.scalars(ids, h, n, "ids"), _plan.scalars(r, h, n * k, "r"), _plan.scalars(alpha, h, 1, "alpha")
    d = bufs.view(engine.fr_sub(_repeat(alpha, n, 1, 32), ids), n, 32)                    # alpha - ID, canonical
    ok = bufs.rows_nonzero(d)
    inv = engine.fr_inverse(bufs.flat(d))
    t = engine.g2_add(engine.g2_scalar_mul_base(engine.fr_neg(r)), _repeat(h, n, k, 128))  # h_j + [-r_j] g2
    hids = engine.g2_scalar_mul(bufs.flat(t), bufs.flat(bufs.expand(bufs.view(inv, n, 1, 32), n, k, 32)))
    rids = bufs.view(r, n, k, 32) * bufs.view(ok, n, 1, 1)
    return rids, bufs.view(hids, n, k, 128), ok


def public_pairings(engine, g1, g2, h):
    """(e_gg [384], e_gh [k, 384]): e(g1, g2) and e(g1, h_j), one pair_batch of 1 + k pairs per public parameters."""
    k = _k_of(bufs.nbytes(h) // 128 if bufs.nbytes(h) % 128 == 0 else 0, "h")
    h = bufs.view(h, k, 128)
    P = _repeat(_plan.public(g1, 1, 64, h, "g1"), 1 + k, 1, 64)
    Q = bufs.flat(bufs.cat([_plan.public(g2, 1, 128, h, "g2"), h], 0))
    e = bufs.view(engine.pair_batch(P, Q), 1 + k, 384)
    return e[0], e[1:]


def encrypt_batch(engine, g1_alpha, e_gg, e_gh, messages, ids, s, gt_table=None):
    """(u [n, 64], v [n, 384], w [n, 384]) and, for k = 3, y [n, 384], for n messages (GT elements, [n, 384]) to n identities (scalars)
    with the randomness s (n scalars).  g1_alpha: g1^alpha; e_gg, e_gh: public_pairings.  u by g1_scalar_mul of the one shared point,
    g1_scalar_mul_base and g1_add; v and e_gh[0]^(-s) by ONE gt_exp over 2 n rows, w by gt_mul; then beta on the device, s beta by
    fr_mul, and y.

    y is two exponentiations — one gt_exp over the 2 n rows (e_gh[1], s), (e_gh[2], s beta) — and a gt_mul, not one gt_multi_exp of
    two-factor segments: gt_multi_exp walks a segment table, n + 1 offsets that would have to be copied to the device for every batch
    (or, made there, be validated with a read-back that stops the stream), and this planner lets nothing per item cross PCIe.  The
    price is the 254 squarings of the second factor, which a shared walk would save.

    gt_table: an engine.GTFixedBase over the 1 + k public pairings in the order e_gg, e_gh[0], ... (engine.GTFixedBase(cat([e_gg,
    e_gh]))).  With it v and e_gh[0]^(-s) are gt_table.pow (32 products each, no squarings) and y is ONE gt_table.indexed with two
    terms per item, the index row (2, 3) shared by all; the bytes are the same.  Without it (the default) the calls are the ones
    above."""
    k = _k_of(bufs.nbytes(e_gh) // 384 if bufs.nbytes(e_gh) % 384 == 0 else 0, "e_gh")
    n = bufs.nbytes(messages) // 384
    if bufs.nbytes(messages) != n * 384:
        raise ValueError("messages are GT elements, rows of 384 bytes")
    messages = bufs.view(messages, n, 384)
    ids, s = _plan.scalars(ids, messages, n, "ids"), _plan.scalars(s, messages, n, "s")
    e_gg, e_gh = _plan.public(e_gg, 1, 384, messages, "e_gg"), _plan.public(e_gh, k, 384, messages, "e_gh")
    neg_s = engine.fr_neg(s)
    u = engine.g1_add(engine.g1_scalar_mul(bufs.flat(_plan.public(g1_alpha, 1, 64, messages, "g1_alpha")), s),
                      engine.g1_scalar_mul_base(engine.fr_mul(bufs.flat(neg_s), ids)))
    if gt_table is None:
        vw = bufs.view(engine.gt_exp(bufs.cat([_repeat(e_gg, n, 1, 384), _repeat(e_gh[0], n, 1, 384)]), bufs.cat([s, bufs.flat(neg_s)])), 2, n, 384)
        v, w_mask = vw[0], vw[1]
    else:
        if gt_table.nbase != 1 + k:
            raise ValueError("gt_table must hold e_gg and the %d e_gh, in that order (it holds %d bases)" % (k, gt_table.nbase))
        v, w_mask = bufs.view(gt_table.pow(s, base=0), n, 384), gt_table.pow(bufs.flat(neg_s), base=1)
    w = engine.gt_mul(bufs.flat(w_mask), bufs.flat(messages))
    out = bufs.view(u, n, 64), v, bufs.view(w, n, 384)
    if k == 1:
        return out
    beta = engine.hash_g1_gt_gt_to_fr(bufs.flat(u), bufs.flat(v), bufs.flat(w))
    s_beta = engine.fr_mul(s, bufs.flat(beta))
    if gt_table is not None:
        exps = bufs.flat(bufs.cat([bufs.view(s, n, 1, 32), bufs.view(s_beta, n, 1, 32)], 1))            # (s, s beta) per item
        return out + (bufs.view(gt_table.indexed(_plan.index_rows(np.array([2, 3]), messages), exps, terms=2)[0], n, 384),)
    yy = bufs.view(engine.gt_exp(bufs.cat([_repeat(e_gh[1], n, 1, 384), _repeat(e_gh[2], n, 1, 384)]), bufs.cat([s, bufs.flat(s_beta)])), 2, n, 384)
    return out + (bufs.view(engine.gt_mul(bufs.flat(yy[0]), bufs.flat(yy[1])), n, 384),)


def decrypt_batch(engine, key, u, v, w, y=None):
    """(messages [n, 384], ok [n]) of n ciphertexts under key = (rids, hids): one key for all of them ([k, 32], [k, 128]) or one per
    ciphertext ([n, k, 32], [n, k, 128]).  k = 3 (y given): beta on the device; e = r_2 + r_3 beta (fr_mul, fr_add);
    Hq = hid_2 + [beta] hid_3 (g2_scalar_mul, g2_add); ONE pair_batch over the 2 n pairs (u, Hq), (u, hid_1) and ONE gt_exp over the
    2 n rows (v, e), (v, r_1); y' = v^e e(u, Hq) and ok = (y' == y) byte for byte — a GT element has one in-memory encoding;
    M = w e(u, hid_1) v^(r_1), all zero where ok = 0 (the reference's "failed to pass decrypt check"), as sw05.decrypt_batch
    leaves a ciphertext it cannot open.  k = 1 (no y): no check, ok is all ones."""
    bufs.device_of(u, v, w, y)
    n = bufs.nbytes(u) // 64
    if bufs.nbytes(u) != n * 64 or bufs.nbytes(v) != n * 384 or bufs.nbytes(w) != n * 384 or (y is not None and bufs.nbytes(y) != n * 384):
        raise ValueError("u, v, w, y must hold n G1, GT, GT and GT elements")
    k = 1 if y is None else 3
    u, v, w = bufs.view(u, n, 64), bufs.view(v, n, 384), bufs.view(w, n, 384)
    rids, hids = key
    rids, hids = _plan.per_item(rids, n, k, 32, u, "rids"), _plan.per_item(hids, n, k, 128, u, "hids")
    if not n:
        return bufs.view(w, 0, 384), bufs.empty((0,), u)
    if k == 1:
        pairs = bufs.view(engine.pair_batch(bufs.flat(u), bufs.flat(hids[:, 0])), n, 384)
        powers = bufs.view(engine.gt_exp(bufs.flat(v), bufs.flat(rids[:, 0])), n, 384)
        ok = bufs.empty((n,), u)
        ok[...] = 1
        return bufs.view(engine.gt_mul(engine.gt_mul(bufs.flat(w), bufs.flat(pairs)), bufs.flat(powers)), n, 384), ok
    beta = bufs.flat(engine.hash_g1_gt_gt_to_fr(bufs.flat(u), bufs.flat(v), bufs.flat(w)))
    e = engine.fr_add(bufs.flat(rids[:, 1]), engine.fr_mul(bufs.flat(rids[:, 2]), beta))
    Hq = engine.g2_add(bufs.flat(hids[:, 1]), engine.g2_scalar_mul(bufs.flat(hids[:, 2]), beta))
    pairs = bufs.view(engine.pair_batch(bufs.cat([bufs.flat(u), bufs.flat(u)]), bufs.cat([bufs.flat(Hq), bufs.flat(hids[:, 0])])), 2, n, 384)
    powers = bufs.view(engine.gt_exp(bufs.cat([bufs.flat(v), bufs.flat(v)]), bufs.cat([bufs.flat(e), bufs.flat(rids[:, 0])])), 2, n, 384)
    ok = bufs.rows_equal(bufs.view(engine.gt_mul(bufs.flat(powers[0]), bufs.flat(pairs[0])), n, 384), bufs.view(y, n, 384))
    m = engine.gt_mul(engine.gt_mul(bufs.flat(w), bufs.flat(pairs[1])), bufs.flat(powers[1]))
    return bufs.view(m, n, 384) * bufs.view(ok, n, 1), ok
