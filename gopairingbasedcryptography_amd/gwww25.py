"""Host-side planner for the batched IBE of Gong, Waters, Wee and Wu (ePrint 2025/2103; bibe/gwww25_bibe/gwww25_bibe.go): KeyGen (:82-128),
Encrypt (:130-160), Digest (:162-176), ComputeKey (:178-209) and Decrypt (:211-256) for many identities, labels and messages at once.  The
scheme mirrors AFP25 with the groups swapped: the SRS powers [tau^i], the digest and the opening proofs live in G2.

What is computed, with the master key (w, v, h, alpha), the SRS secret tau, an identity id, a batch label tg and randomness s, r, y in Zr:

    KeyGen       [tau^i]_2, i = 1 .. B     [tau]_1  [w]_1  [w tau]_1  [v]_1  [h]_1     [alpha]_T = e(g1, g2)^alpha
    Encrypt      ct1 = [s]_1     ct2 = s [w tau]_1 - (s id) [w]_1     ct3 = s ([v]_1 + tg [h]_1)     ct4 = [alpha]_T^s M
    Digest       D = [f(tau)]_2,  f(X) = prod over the batch's 1 <= m <= B identities of (X - id)
    ComputeKey   u1 = [r]_2     u2 = (y w) D + [alpha + r (v + h tg)]_2     the key is (y, u1, u2)
    Decrypt      pi = [f(tau) / (tau - id)]_2     M = ct4 / (e(ct1, u2) / e(y ct2, pi) / e(ct3, u1))

A batch holds any number of identities from 1 to B (Digest, :163-168), so every function that takes identities takes `counts`, the batch
sizes, beside them.  The opening proofs come from engine.FixedBase.openings over the SRS table (srs_table: g2, [tau]_2 .. [tau^B]_2): the
quotient's coefficients are made in the lane that adds their terms, and the reference's rule that the identity occurs exactly once in its
batch (:214-223) is decided on the device as ok = 0 with an all-zero message, where the reference returns an error.  The quotient of
Decrypt folds into the pairing exactly — e(P, Q)^-1 = e(-P, Q) as Fp12 elements — so an item costs one multi-pairing segment of three
pairs, (ct1, u2), (-y ct2, pi), (-ct3, u1), and one GT division.  The two fmt.Printf calls of the reference (:171, :225) have no
counterpart.

Host orchestration only, engine-agnostic (every function takes the engine: `bn254`, or a stand-in with the same names).  Randomness comes
in as arguments (scalar rows, or Python integers); the *_seeded forms draw it from an rng.Randomness.  Host arrays in give host arrays
out; CUDA tensors in give CUDA tensors out."""
import numpy as np

from . import _buffers as bufs, _plan
from ._buffers import R_ORDER

MAX_B = 1024          # FR_POLY_MAX_B: the longest batch the polynomial kernels take
MPK_G1 = ("G1ExpTau", "G1ExpW", "G1ExpWTau", "G1ExpV", "G1ExpH")


def _int(v, what):
    """one scalar as a Python integer modulo r: an integer, or one scalar row"""
    if _plan.is_buffer(v):
        if bufs.nbytes(v) != 32:
            raise ValueError("%s must be one scalar" % what)
        v = int.from_bytes(np.asarray(v.cpu() if bufs.is_torch(v) else v, dtype=np.uint8).tobytes(), "little")
    return int(v) % R_ORDER


def keygen(engine, B, tau, w, v, h, alpha):
    """mpk (KeyGen, :82-128) as a dict of host arrays: G2ExpTauPowers [B, 128] = [tau]_2 .. [tau^B]_2, G1ExpTau, G1ExpW, G1ExpWTau, G1ExpV,
    G1ExpH [64] each, GTExpAlpha [384] = gt_exp(pair(g1, g2), alpha).  The master secret key is the caller's (w, v, h, alpha).  The B <=
    1024 powers of tau are computed in Python integers, then ONE g2_scalar_mul_base; the five G1 values are one g1_scalar_mul_base."""
    if not isinstance(B, (int, np.integer)) or isinstance(B, bool) or not 1 <= B <= MAX_B:
        raise ValueError("invalid B")                                          # Setup, :73-80, and the polynomial kernels' limit
    tau, w, v, h, alpha = (_int(x, name) for x, name in zip((tau, w, v, h, alpha), ("tau", "w", "v", "h", "alpha")))
    g1, g2 = engine.generators()
    in_g1 = bufs.view(engine.g1_scalar_mul_base(bufs.flat(_plan.scalar_rows([tau, w, tau * w % R_ORDER, v, h]))), 5, 64)
    powers = bufs.view(engine.g2_scalar_mul_base(bufs.flat(_plan.scalar_rows([pow(tau, i, R_ORDER) for i in range(1, int(B) + 1)]))), int(B), 128)
    e = engine.pair_batch(np.asarray(g1, dtype=np.uint8).reshape(-1), np.asarray(g2, dtype=np.uint8).reshape(-1))
    mpk = {name: np.array(in_g1[i], dtype=np.uint8, copy=True) for i, name in enumerate(MPK_G1)}
    mpk["G2ExpTauPowers"] = np.array(powers, dtype=np.uint8, copy=True)
    mpk["GTExpAlpha"] = np.array(bufs.view(engine.gt_exp(bufs.flat(e), bufs.flat(_plan.scalar_rows([alpha]))), 384), dtype=np.uint8, copy=True)
    return mpk


def keygen_seeded(engine, B, rng):
    """(mpk, (w, v, h, alpha)): keygen on ONE draw of five scalars in the reference's order, tau, w, v, h, alpha (:83-91).  tau is used
    and dropped.  The seed is key material."""
    drawn = np.asarray(rng.scalars(np.zeros(0, dtype=np.uint8), 5), dtype=np.uint8).reshape(5, 32)
    tau, w, v, h, alpha = (int.from_bytes(r.tobytes(), "little") for r in drawn)
    return keygen(engine, B, tau, w, v, h, alpha), (w, v, h, alpha)


def srs_table(engine, mpk):
    """engine.FixedBase over (g2, [tau]_2, ..., [tau^B]_2), g2=True: base c stands for [tau^c]_2.  Built once per master public key."""
    _, g2 = engine.generators()
    powers = np.asarray(mpk["G2ExpTauPowers"], dtype=np.uint8).reshape(-1, 128)
    return engine.FixedBase(np.concatenate([np.asarray(g2, dtype=np.uint8).reshape(1, 128), powers]), g2=True)


def encrypt_tables(engine, mpk):
    """(g1_table, gt_table) for encrypt_batch: an engine.FixedBase over ([w tau]_1, -[w]_1, [v]_1, [h]_1) and an engine.GTFixedBase over
    [alpha]_T.  With them ct2 and ct3 are two indexed sums of two terms and [alpha]_T^s is 32 products."""
    neg_w = np.asarray(engine.g1_neg(np.asarray(mpk["G1ExpW"], dtype=np.uint8).reshape(64)), dtype=np.uint8).reshape(1, 64)
    g1_bases = np.concatenate([np.asarray(mpk["G1ExpWTau"], dtype=np.uint8).reshape(1, 64), neg_w] + [np.asarray(mpk[k], dtype=np.uint8).reshape(1, 64) for k in ("G1ExpV", "G1ExpH")])
    return engine.FixedBase(g1_bases), engine.GTFixedBase(np.asarray(mpk["GTExpAlpha"], dtype=np.uint8).reshape(384))


def _pairs_of(a, b, n):
    """[n * 2 * 32] flat: the scalars (a[i], b[i]) of n two-term sums"""
    return bufs.flat(bufs.cat([bufs.view(a, n, 1, 32), bufs.view(b, n, 1, 32)], 1))


def encrypt_batch(engine, mpk, messages, ids, tg, s, tables=None):
    """(ct1 [n, 64], ct2 [n, 64], ct3 [n, 64], ct4 [n, 384]) for n messages (GT elements) to n identities under the label tg — one for
    all, or one per item — with the randomness s (Encrypt, :130-160).
    Without tables the reference's operations in the reference's order: g1_scalar_mul_base(s); g1_scalar_mul of the one [w tau]_1 by s
    and of the one [w]_1 by fr_mul(s, id), g1_sub; g1_scalar_mul of [h]_1 by tg, g1_add to [v]_1, g1_scalar_mul by s; gt_exp and gt_mul.
    With tables = encrypt_tables(...): ct2 = indexed(terms=2) over ([w tau]_1; s), (-[w]_1; s id), ct3 = indexed(terms=2) over ([v]_1; s),
    ([h]_1; s tg), ct4 = gt_mul(gt_table.pow(s), M).  The bytes are the same either way."""
    n = bufs.nbytes(messages) // 384
    if bufs.nbytes(messages) != n * 384:
        raise ValueError("messages are GT elements, rows of 384 bytes")
    messages = bufs.view(messages, n, 384)
    ids, s = _plan.scalars(ids, messages, n, "ids"), _plan.scalars(s, messages, n, "s")
    tg = _plan.scalars(tg, messages)
    if bufs.is_torch(tg) != bufs.is_torch(messages) or bufs.nbytes(tg) not in (32, n * 32):
        raise ValueError("tg must hold one label, or one per item, of the kind the other arguments are")
    tg = bufs.flat(bufs.view(tg, -1))
    if not n:
        return bufs.empty((0, 64), messages), bufs.empty((0, 64), messages), bufs.empty((0, 64), messages), messages
    ct1 = engine.g1_scalar_mul_base(s)
    sid = bufs.flat(engine.fr_mul(s, ids))
    if tables is None:
        pub = {k: bufs.flat(_plan.public(mpk[k], 1, 64, messages, k)) for k in ("G1ExpWTau", "G1ExpW", "G1ExpV", "G1ExpH")}
        ct2 = engine.g1_sub(engine.g1_scalar_mul(pub["G1ExpWTau"], s), engine.g1_scalar_mul(pub["G1ExpW"], sid))
        v_tgh = engine.g1_add(engine.g1_scalar_mul(pub["G1ExpH"], tg), pub["G1ExpV"])              # one point per label
        ct3 = engine.g1_scalar_mul(bufs.flat(v_tgh), s)
        ct4 = _plan.blind(engine, _plan.public(mpk["GTExpAlpha"], 1, 384, messages, "GTExpAlpha"), s, messages, n)
    else:
        g1_table, gt_table = tables
        if g1_table.nbase != 4 or gt_table.nbase != 1:
            raise ValueError("tables are encrypt_tables(engine, mpk): four G1 bases and one GT base")
        stg = bufs.flat(engine.fr_mul(s, tg))
        ct2 = g1_table.indexed(_plan.index_rows(np.array([[0, 1]]), messages), _pairs_of(s, sid, n), terms=2)[0]
        ct3 = g1_table.indexed(_plan.index_rows(np.array([[2, 3]]), messages), _pairs_of(s, stg, n), terms=2)[0]
        ct4 = engine.gt_mul(bufs.flat(gt_table.pow(s)), bufs.flat(messages))
    return bufs.view(ct1, n, 64), bufs.view(ct2, n, 64), bufs.view(ct3, n, 64), bufs.view(ct4, n, 384)


def encrypt_batch_seeded(engine, mpk, messages, ids, tg, rng, tables=None):
    """encrypt_batch with its randomness drawn on the device: ONE draw, s [n] — one stream id, none when n == 0 — of the kind the messages
    are; the return value is exactly encrypt_batch's on the scalars drawn.  The seed is key material."""
    return encrypt_batch(engine, mpk, messages, ids, tg, rng.scalars(messages, bufs.nbytes(messages) // 384), tables)


def _batches(table, ids, counts):
    """(flat identity rows, counts) with the reference's two refusals (Digest, :163-168): an empty batch, a batch longer than B"""
    counts = [int(c) for c in counts]
    if not counts or any(c == 0 for c in counts):
        raise ValueError("identities is empty")
    if any(c < 0 or c > table.nbase - 1 for c in counts):
        raise ValueError("too many identities for batch size")
    ids = ids if _plan.is_buffer(ids) else _plan.scalar_rows(ids)
    if bufs.nbytes(ids) != sum(counts) * 32:
        raise ValueError("ids must hold one scalar per identity of every batch (%d)" % sum(counts))
    return bufs.flat(bufs.view(ids, -1)), counts


def digests(engine, table, ids, counts):
    """D [k, 128], D_j = [f_j(tau)]_2 for k batches of counts[j] identities each (Digest, :162-176): one kernel expands every f_j into a
    row of table.nbase scalars, one fixed-base MSM row per batch commits to it.  table: srs_table.  An empty batch raises
    ValueError("identities is empty"), one longer than B ValueError("too many identities for batch size"), as the reference."""
    ids, counts = _batches(table, ids, counts)
    coeffs = engine.fr_poly_from_roots_segments(ids, counts, table.nbase)
    return bufs.view(table.msm(bufs.flat(coeffs)), len(counts), 128)


def compute_key_batch(engine, msk, D, tg, r, y):
    """(y [k, 32], u1 [k, 128], u2 [k, 128]) for k (digest, label) pairs with the randomness r, y (ComputeKey, :178-209): u1 by
    g2_scalar_mul_base(r); u2 by fr_mul(y, w), g2_scalar_mul(D, y w), then h tg, + v, times r, + alpha in Fr, g2_scalar_mul_base and
    g2_add.  msk = (w, v, h, alpha); tg: one label per pair, or one for all."""
    k = bufs.nbytes(D) // 128
    if bufs.nbytes(D) != k * 128:
        raise ValueError("D holds G2 points, rows of 128 bytes")
    D = bufs.view(D, k, 128)
    w, v, h, alpha = (_plan.scalars(x, D, 1, name) for x, name in zip(msk, ("w", "v", "h", "alpha")))
    r, y = _plan.scalars(r, D, k, "r"), _plan.scalars(y, D, k, "y")
    tg = _plan.scalars(tg, D)
    if bufs.is_torch(tg) != bufs.is_torch(D) or bufs.nbytes(tg) not in (32, k * 32):
        raise ValueError("tg must hold one label, or one per digest, of the kind the other arguments are")
    if not k:
        return bufs.empty((0, 32), D), bufs.empty((0, 128), D), D
    tg = bufs.flat(bufs.expand(bufs.view(tg, -1, 32), k, 32))
    u1 = engine.g2_scalar_mul_base(r)
    ywd = engine.g2_scalar_mul(bufs.flat(D), bufs.flat(engine.fr_mul(y, w)))
    t = engine.fr_add(engine.fr_mul(tg, h), v)                                 # v + h tg
    t = engine.fr_add(engine.fr_mul(r, bufs.flat(t)), alpha)                   # alpha + r (v + h tg)
    u2 = engine.g2_add(ywd, engine.g2_scalar_mul_base(bufs.flat(t)))
    return bufs.view(y, k, 32), bufs.view(u1, k, 128), bufs.view(u2, k, 128)


def compute_key_batch_seeded(engine, msk, D, tg, rng):
    """compute_key_batch with its randomness drawn on the device: TWO draws, r [k] then y [k], the reference's order (:179-186).  The
    seed is key material."""
    k = bufs.nbytes(D) // 128
    r = rng.scalars(D, k)
    return compute_key_batch(engine, msk, D, tg, r, rng.scalars(D, k))


def decrypt_batches(engine, table, ids, counts, sk, ct, coeffs=None):
    """(messages [n, 384], ok [n]) for the n identities of k batches (Decrypt, :211-256).  table: srs_table; ids, counts: the batches as
    digests takes them, every identity with its ciphertext ct = (ct1, ct2, ct3, ct4), n rows each; sk = (y, u1, u2) with one row per
    batch (k) or per item (n).  pi, ok = table.openings(ids, counts); y ct2 by g1_scalar_mul; ONE multi_pair over the 3-pair segments
    (ct1, u2), (-y ct2, pi), (-ct3, u1); gt_div(ct4, .) — the Fp12 element of the reference's three Pair and three Div.  An identity
    that does not occur exactly once in its batch (the reference's error, :221-223) has ok = 0 and an all-zero message.  coeffs: the
    batch polynomials as engine.fr_poly_from_roots_segments(ids, counts, table.nbase) gives them, when the caller has them from the
    digests (made by table.openings when None); an identity that is no root of its row has ok = 0.  Nothing here reads a result back: ok
    stays where the batch lives (multi_pair's own self-check is the engine's)."""
    ids, counts = _batches(table, ids, counts)
    n, k = sum(counts), len(counts)
    ct1, ct2, ct3 = (bufs.view(x, -1, 64) for x in ct[:3])
    ct4 = bufs.view(ct[3], -1, 384)
    if any(x.shape[0] != n for x in (ct1, ct2, ct3, ct4)) or bufs.is_torch(ct4) != bufs.is_torch(ids):
        raise ValueError("every ciphertext component must hold one row per identity (%d), of the kind the identities are" % n)
    of_item = np.repeat(np.arange(k), counts)

    def per_item(x, width, name):
        x = _plan.scalars(x, ct4) if width == 32 else x
        if bufs.is_torch(x) != bufs.is_torch(ct4) or bufs.nbytes(x) not in (k * width, n * width):
            raise ValueError("%s must hold one row of %d bytes per batch (%d) or per item (%d)" % (name, width, k, n))
        x = bufs.view(x, -1, width)
        return x if x.shape[0] == n else bufs.take(x, of_item)
    y, u1, u2 = per_item(sk[0], 32, "y"), per_item(sk[1], 128, "u1"), per_item(sk[2], 128, "u2")
    pi, ok = table.openings(ids, counts) if coeffs is None else table.openings(ids, counts, coeffs=bufs.flat(coeffs))
    yct2 = engine.g1_scalar_mul(bufs.flat(ct2), bufs.flat(y))
    zero = bufs.zeros((n * 64,), ct4)
    P = _plan.interleave([bufs.flat(ct1), engine.g1_sub(zero, bufs.flat(yct2)), engine.g1_sub(zero, bufs.flat(ct3))], 64)
    Q = _plan.interleave([bufs.flat(u2), bufs.flat(pi), bufs.flat(u1)], 128)
    m = bufs.view(engine.gt_div(bufs.flat(ct4), bufs.flat(engine.multi_pair(P, Q, _plan.segments(n, 3)))), n, 384)
    return m * bufs.view(ok, n, 1), ok
