"""Host-side planner for batched LW11 decentralised ABE decryption (Lewko-Waters 2011; dabe/lw11_dabe.go:176-203): one user key,
one LSSS policy, a batch of ciphertexts under that policy.

What is computed.  With the rows x whose attribute rho(x) the user holds and weights w_x such that sum_x w_x M_x = (1, 0, ..., 0),

    M = c0 / prod_x ( c1x * e(H(GID), c3x) / e(K_rho(x),GID, c2x) ) ^ w_x

because c1x e(H, c3x) / e(K, c2x) = e(g1, g2)^lambda_x e(H, g2)^omega_x, and the shares recombine to sum w_x lambda_x = s,
sum w_x omega_x = 0.  Two of the three factors fold into the key, once per (key, policy): e(H, c3x)^w = e([w]H, c3x) and
e(K, c2x)^-w = e([-w]K, c2x) exactly as Fp12 elements, so per ciphertext

    E = Pair([A_x..., B_x...], [c3x..., c2x...]),  A_x = [w_x] H(GID),  B_x = [-w_x] K_rho(x),GID     one multi-pairing segment of 2k pairs
    F = prod_x c1x ^ w_x                                                                             one GT multi-exponentiation
    M = c0 / (E * F)

c1x is ciphertext data in GT: it cannot be folded into a key or in front of a pairing, which is why this scheme needs a product of
powers of varying GT bases per ciphertext (engine.gt_multi_exp with ONE exponent list for all ciphertexts).

The pairings against H(GID) fold further by bilinearity, prod_x e([w_x]H, c3x) = e(H, sum_x w_x c3x): decrypt_batch_msm takes the sum
from engine.g2_multi_scalar_mul (the weights as ONE scalar list for all ciphertexts) and spends k + 1 pairings per ciphertext where
decrypt_batch spends 2k; the messages are the same bytes.

The reference's loop is not that formula: it raises the RUNNING product to the weight at every row, ((1 * t_0)^w * t_1)^w' ...,
and it indexes the compacted weight slice by the matrix row number (lw11_dabe.go:191-195; SURVEY.md's notes on Waters11 / DABE
record both).  The two agree when every weight is 1 — the solution that Lewko-Waters matrices of AND / OR formulas have — and this
planner follows the scheme, not the loop, just as bsw07.py drops the reference's debug pairing.

The other end of the scheme is here too: authority_setup (the public keys of an authority's attributes), keygen_batch (the keys of U
users over A attributes: one H(GID) per user raised to the row of the authority's y_i, the row form of engine.g1_scalar_mul) and
encrypt_batch, each with a *_seeded form where it draws randomness.

Host orchestration only, engine-agnostic (every function takes the engine: `bn254`, or a stand-in with the same function names):
the elimination is per policy, microseconds in Python integers, and stays on the host."""
import numpy as np

from . import _buffers as bufs, _plan
from ._buffers import R_ORDER
from ._plan import INDEX_NONE      # noqa: F401 (for callers that build index rows themselves)


def reconstruction_weights(matrix, rho, attributes):
    """(rows, weights): the rows x with rho[x] in `attributes` that carry a non-zero weight, and w_x in [1, r) with
    sum_x w_x matrix[x] = (1, 0, ..., 0) modulo r; None when the attribute set does not satisfy the policy
    (FindLinearCombinationWeight, access/lsss/lewko_waters_lsss_matrix.go:167-221).  Gauss-Jordan elimination on the transposed
    sub-matrix; unknowns without a pivot (redundant rows) get weight 0 and are dropped."""
    attrs = set(attributes)
    sat = [x for x in range(len(rho)) if rho[x] in attrs]
    if not sat:
        return None
    cols = len(matrix[0])
    m = len(sat)
    aug = [[int(matrix[x][j]) % R_ORDER for x in sat] + [1 if j == 0 else 0] for j in range(cols)]     # cols equations, m unknowns
    pivots, row = [], 0
    for col in range(m):
        p = next((i for i in range(row, cols) if aug[i][col]), None)
        if p is None:
            continue
        aug[row], aug[p] = aug[p], aug[row]
        inv = pow(aug[row][col], -1, R_ORDER)
        aug[row] = [v * inv % R_ORDER for v in aug[row]]
        for i in range(cols):
            if i != row and aug[i][col]:
                f = aug[i][col]
                aug[i] = [(a - f * b) % R_ORDER for a, b in zip(aug[i], aug[row])]
        pivots.append(col)
        row += 1
        if row == cols:
            break
    if any(aug[i][m] for i in range(row, cols)):                 # 0 = non-zero: the target is not in the span
        return None
    w = [0] * m
    for i, col in enumerate(pivots):
        w[col] = aug[i][m]
    rows = [sat[i] for i in range(m) if w[i]]
    weights = [w[i] for i in range(m) if w[i]]
    for j in range(cols):                                          # the defining identity, checked on what is returned
        assert sum(wx * int(matrix[x][j]) for x, wx in zip(rows, weights)) % R_ORDER == (1 if j == 0 else 0)
    return rows, weights


def fold_key(engine, rows, weights, h_gid, k_by_rho):
    """Once per (key, policy): A_x = [w_x] H(GID) and B_x = [-w_x] K_rho(x),GID for the used rows.
    h_gid: the 64-byte H(GID); k_by_rho[x]: the 64-byte key component of row x's attribute (a mapping or a sequence indexed by the
    matrix row).  Returns (rows, weights, A [k, 64], B [k, 64])."""
    if len(rows) != len(weights) or not rows:
        raise ValueError("one weight per used row, at least one row")
    h = np.asarray(h_gid, dtype=np.uint8).reshape(64)
    kb = np.stack([np.asarray(k_by_rho[x], dtype=np.uint8).reshape(64) for x in rows])
    A = engine.g1_scalar_mul(np.stack([h] * len(rows)), [int(w) % R_ORDER for w in weights])
    B = engine.g1_scalar_mul(kb, [(-int(w)) % R_ORDER for w in weights])
    return list(rows), [int(w) % R_ORDER for w in weights], np.asarray(A).reshape(-1, 64), np.asarray(B).reshape(-1, 64)


def decrypt_batch(engine, folded, c0, c1, c2, c3):
    """The n messages of n ciphertexts under one folded (key, policy): c0 [n, 384]; c1 [n, R, 384], c2, c3 [n, R, 128] with all R
    rows of the policy per ciphertext (the used rows are picked here).  numpy in, numpy out; CUDA tensors in, CUDA tensor out, with
    only the folded key, the weights and a segment table going to the device.  Three engine calls besides the row selection:
    multi_pair (n segments of 2k pairs, one final exponentiation each), gt_multi_exp with the shared weight list, and
    gt_mul + gt_div."""
    rows, weights, A, B = folded
    k = len(rows)
    bufs.device_of(c0, c1, c2, c3)                                           # one kind of buffer, one device
    n = bufs.nbytes(c0) // 384

    def used(c, width):
        """the used rows of a per-row component: [n, k, width]"""
        return bufs.take(bufs.view(c, n, -1, width), rows, 1)
    P = bufs.expand(bufs.put(np.concatenate([A, B]).reshape(1, 2 * k, 64), c0), n, 2 * k, 64)
    Q = bufs.cat([used(c3, 128), used(c2, 128)], 1)
    E = engine.multi_pair(bufs.flat(P), bufs.flat(Q), _plan.segments(n, 2 * k))
    F = engine.gt_multi_exp(bufs.flat(used(c1, 384)), weights, _plan.segments(n, k))
    return engine.gt_div(bufs.flat(c0).reshape(n, 384), engine.gt_mul(E, F))


def decrypt_batch_msm(engine, folded, h_gid, c0, c1, c2, c3):
    """decrypt_batch with the k pairings against H(GID) folded into one: E = Pair([H, B_x...], [sum_x w_x c3x, c2x...]), one segment
    of k + 1 pairs per ciphertext, the sum from engine.g2_multi_scalar_mul with the shared weight list (n segments of k terms).  F and
    the division are decrypt_batch's, and so are the messages, byte for byte (bilinearity, canonical GT output).  h_gid: the 64-byte
    H(GID) that fold_key was given."""
    rows, weights, _, B = folded
    k = len(rows)
    bufs.device_of(c0, c1, c2, c3)                                           # one kind of buffer, one device
    n = bufs.nbytes(c0) // 384

    def used(c, width):
        return bufs.take(bufs.view(c, n, -1, width), rows, 1)
    table = _plan.segments(n, k)
    S = engine.g2_multi_scalar_mul(bufs.flat(used(c3, 128)), weights, table).reshape(n, 1, 128)
    hb = np.concatenate([np.asarray(h_gid, dtype=np.uint8).reshape(1, 64), B])
    P = bufs.expand(bufs.put(hb.reshape(1, k + 1, 64), c0), n, k + 1, 64)
    Q = bufs.cat([S, used(c2, 128)], 1)
    E = engine.multi_pair(bufs.flat(P), bufs.flat(Q), _plan.segments(n, k + 1))
    F = engine.gt_multi_exp(bufs.flat(used(c1, 384)), weights, table)
    return engine.gt_div(bufs.flat(c0).reshape(n, 384), engine.gt_mul(E, F))


# ------------------------------------------------------------------------------------------------ AuthoritySetup, KeyGenerate
def _secrets(alpha, y):
    """(alpha, y, A): an authority's secrets as flat scalar buffers of one kind — that of whichever is a buffer, host arrays otherwise"""
    like = next((x for x in (alpha, y) if _plan.is_buffer(x)), np.zeros(0, dtype=np.uint8))
    alpha, y = _plan.scalars(alpha, like), _plan.scalars(y, like)
    bufs.device_of(alpha, y)
    A = bufs.nbytes(alpha) // 32
    if bufs.nbytes(alpha) != A * 32 or bufs.nbytes(y) != A * 32:
        raise ValueError("alpha and y must hold one 32-byte scalar per attribute each (got %d and %d bytes)" % (bufs.nbytes(alpha), bufs.nbytes(y)))
    return bufs.flat(alpha), bufs.flat(y), A


def authority_setup(engine, e, alpha, y, gt_table=None):
    """The public keys of A attributes from their secrets (AuthoritySetup, dabe/lw11_dabe.go:63-88): (egg_alpha [A, 384], g2_y [A, 128])
    with egg_alpha_i = e(g1, g2)^alpha_i and g2_y_i = [y_i] g2.  e = e(g1, g2) (384 B); alpha, y: A scalars each, Python ints, uint8
    arrays or CUDA tensors (the outputs are of their kind).  gt_table: an engine.GTFixedBase whose base 0 is e, built once by the
    caller; the powers then come from its indexed products and are the same bytes.  Engine calls: gt_exp on e repeated (or
    gt_table.indexed, one term) and g2_scalar_mul_base.  Rows i of the two results are the values of encrypt_batch's dictionaries."""
    alpha, y, A = _secrets(alpha, y)
    if not A:
        return bufs.zeros((0, 384), alpha), bufs.zeros((0, 128), alpha)
    if gt_table is None:
        base = _plan.public(e, 1, 384, alpha, "e")
        egg = engine.gt_exp(bufs.flat(bufs.expand(base, A, 384)), alpha)
    else:
        egg, _ = gt_table.indexed(_plan.index_rows(np.array([[0]]), alpha), alpha, terms=1)
    return bufs.view(egg, A, 384), bufs.view(engine.g2_scalar_mul_base(y), A, 128)


def authority_setup_seeded(engine, e, n_attrs, rng, like=None, gt_table=None):
    """(alpha [A, 32], y [A, 32], egg_alpha, g2_y): authority_setup with the secrets of A = n_attrs attributes drawn on the device; rng is
    an rng.Randomness over the engine.  The draws, in this order (the order is part of the interface: it is what makes the keys
    reproducible from the seed): alpha [A], then y [A] — two stream ids, none when A == 0.  like: a buffer of the kind the secrets and
    the keys are to be (None: host arrays).  The seed is key material: whoever holds it holds the authority's secret key."""
    like = np.zeros(0, dtype=np.uint8) if like is None else like
    alpha = rng.scalars(like, n_attrs)
    y = rng.scalars(like, n_attrs)
    return (alpha, y) + authority_setup(engine, e, alpha, y, gt_table=gt_table)


def keygen_batch(engine, gids, alpha, y, mask=None, h_gid=None):
    """The keys of U users over A attributes (KeyGenerate, dabe/lw11_dabe.go:90-107): K [U, A, 64] with
    K[u, i] = [alpha_i] g1 + [y_i] H(GID_u).  gids: the U global identifiers, str (hashed as UTF-8, hash.ToG1) or bytes, hashed by
    engine.hash_to_g1 with the reference's tag; or None with h_gid [U, 64], the rows H(GID_u) ready (numpy, or CUDA tensors: everything
    then stays on the device).  alpha, y: the authority's A secrets each (Python ints, uint8 arrays or tensors of h_gid's kind).
    mask [U, A] bytes: non-zero = user u is granted attribute i; the other rows of K come out all zero (None: every attribute to every
    user).  Engine calls: hash_to_g1, g1_scalar_mul in its ROW form — U bases, U * A scalars, y repeated per user, row-major: one
    base per user and a row of A scalars per base —, g1_scalar_mul_base of the A alphas, g1_add.  K[u] indexed by the matrix rows'
    attributes is the k_by_rho of fold_key."""
    if h_gid is None:
        if gids is None:
            raise ValueError("need the identifiers gids, or their hashes h_gid")
        from .hash_to import DST_STRING_G1
        h_gid = engine.hash_to_g1([g.encode("utf-8") if isinstance(g, str) else bytes(g) for g in gids], DST_STRING_G1)
        h_gid = bufs.put(h_gid, next((x for x in (alpha, y) if bufs.is_torch(x)), h_gid))      # the hashes go where the secrets live
    U = bufs.nbytes(h_gid) // 64
    if bufs.nbytes(h_gid) != U * 64:
        raise ValueError("h_gid must hold whole G1 points")
    h = bufs.view(h_gid, U, 64)
    alpha, y = (_plan.scalars(x, h) for x in (alpha, y))
    bufs.device_of(h, alpha, y)
    A = bufs.nbytes(alpha) // 32
    if bufs.nbytes(alpha) != A * 32 or bufs.nbytes(y) != A * 32:
        raise ValueError("alpha and y must hold one 32-byte scalar per attribute each")
    if mask is not None:
        mask = _plan.public(mask, U * A, 1, h, "mask")
    if not U or not A:
        return bufs.zeros((U, A, 64), h)
    T = engine.g1_scalar_mul(bufs.flat(h), bufs.flat(bufs.expand(bufs.view(y, 1, A, 32), U, A, 32)))
    ga = engine.g1_scalar_mul_base(bufs.flat(alpha))
    K = bufs.view(engine.g1_add(bufs.flat(T), bufs.flat(bufs.expand(bufs.view(ga, 1, A, 64), U, A, 64))), U * A, 64)
    if mask is not None:
        K = K * bufs.view(bufs.rows_nonzero(mask), U * A, 1)
    return bufs.view(K, U, A, 64)


# ------------------------------------------------------------------------------------------------ Encrypt
def encrypt_table(engine, g2_y, g2=None):
    """The G2 fixed-base table of encrypt_batch over (g2, g2^y_u ...), u in ascending order: built once, passed as `table` to any number
    of calls, closed by the caller.  g2: the generator's 128 bytes (None: engine.generators()[1])."""
    attrs = sorted(g2_y)
    gen = np.asarray(engine.generators()[1] if g2 is None else g2, dtype=np.uint8).reshape(128)
    return engine.FixedBase(np.stack([gen] + [np.asarray(g2_y[u], dtype=np.uint8).reshape(128) for u in attrs]), g2=True)


def encrypt_batch(engine, e, egg_alpha, g2_y, matrix, rho, messages, s, v, w, r, table=None):
    """n ciphertexts under one policy (Encrypt, dabe/lw11_dabe.go:100-174).  e = e(g1, g2) (384 B); egg_alpha: {attribute:
    e(g1, g2)^alpha_u (384 B)} and g2_y: {attribute: g2^y_u (128 B)}, the authorities' public keys; (matrix, rho): the policy, R rows and
    C columns; messages [n, 384]; s: n scalars; v, w: [n, C - 1] scalars, the rest of the share vectors (s, v_2, ..) and (0, w_2, ..);
    r: [n, R] scalars.  Scalars are Python ints, uint8 arrays or CUDA tensors.

    The shares are taken over every ROW of the matrix, lambda_x = M_x . (s, v) and omega_x = M_x . (0, w), as the scheme and
    decrypt_batch have it; the reference's loop runs to ColumnNumber() (lw11_dabe.go:111,139), which covers every row only for a square
    matrix.

    Returns exactly the operands of decrypt_batch: (c0 [n, 384], c1 [n, R, 384], c2 [n, R, 128], c3 [n, R, 128]) with
    c0 = M e^s, c1x = e^lambda_x (e^alpha_rho(x))^r_x, c2x = [r_x] g2, c3x = [r_x] g2^y_rho(x) + [omega_x] g2.  An attribute of rho
    without a public key is a ValueError (the reference's attribute check).  table: encrypt_table(engine, g2_y) built once by the
    caller; None builds and closes one here.  Engine calls: fr_lsss_shares twice (one matrix for the batch), gt_multi_exp over n R
    segments of two factors, g2_scalar_mul_base, FixedBase.indexed (G2, terms = 2, the R index rows periodic), gt_exp, gt_mul."""
    R, C = len(matrix), len(matrix[0]) if len(matrix) else 0
    if not R or not C or len(rho) != R or any(len(row) != C for row in matrix):
        raise ValueError("the policy needs R >= 1 rows of C >= 1 entries and one attribute per row")
    attrs = sorted(g2_y)
    where = {u: i for i, u in enumerate(attrs)}
    for u in rho:
        if u not in where or u not in egg_alpha:
            raise ValueError("attribute %s is not in the universe" % (u,))
    n = bufs.nbytes(messages) // 384
    if bufs.nbytes(messages) != n * 384:
        raise ValueError("messages must hold whole GT elements")
    s, v, w, r = (x if x is None else _plan.scalars(x, messages) for x in (s, v, w, r))
    bufs.device_of(messages, s, v, w, r)                                       # one kind of buffer, one device
    size = lambda x: 0 if x is None else bufs.nbytes(x)
    if size(s) != n * 32 or size(v) != n * (C - 1) * 32 or size(w) != n * (C - 1) * 32 or size(r) != n * R * 32:
        raise ValueError("need s [n], v and w [n, C - 1], r [n, R] scalars with n = %d, R = %d, C = %d" % (n, R, C))
    if not n:
        z = lambda *shape: bufs.zeros(shape, messages)
        return z(0, 384), z(0, R, 384), z(0, R, 128), z(0, R, 128)
    put = lambda a: bufs.put(np.ascontiguousarray(a), messages)
    s3 = bufs.view(s, n, 1, 32)
    mat = put(_plan.scalar_rows(x for row in matrix for x in row).reshape(-1))
    vec_s = s3 if C == 1 else bufs.cat([s3, bufs.view(v, n, C - 1, 32)], 1)
    vec_0 = bufs.zeros((n, 1, 32), messages) if C == 1 else bufs.cat([bufs.zeros((n, 1, 32), messages), bufs.view(w, n, C - 1, 32)], 1)
    lam = engine.fr_lsss_shares(mat, bufs.flat(vec_s), R, C)                   # [n, R, 32]
    om = engine.fr_lsss_shares(mat, bufs.flat(vec_0), R, C)
    r2 = bufs.view(r, n * R, 1, 32)
    # c1x = e^lambda_x (e^alpha_rho(x))^r_x: one segment of two factors per (ciphertext, row)
    pairs = np.stack([np.stack([np.asarray(e, dtype=np.uint8).reshape(384), np.asarray(egg_alpha[u], dtype=np.uint8).reshape(384)]) for u in rho])     # [R, 2, 384]
    gt_bases = bufs.flat(bufs.expand(bufs.view(put(pairs), 1, 2 * R, 384), n, 2 * R, 384))
    c1 = engine.gt_multi_exp(gt_bases, bufs.flat(bufs.cat([bufs.view(lam, n * R, 1, 32), r2], 1)), _plan.segments(n * R, 2))
    c2 = engine.g2_scalar_mul_base(bufs.flat(r))
    # c3x = [r_x] g2^y_rho(x) + [omega_x] g2: base 0 is g2, base 1 + i the i-th public key; the R index rows repeat per ciphertext
    index = _plan.index_rows(np.array([[1 + where[u], 0] for u in rho]), messages)
    with _plan.handle(table, lambda: encrypt_table(engine, g2_y), "nbase", 1 + len(attrs), "the table holds %(got)d bases, the public keys need %(want)d") as table:
        c3, ok = table.indexed(index, bufs.flat(bufs.cat([r2, bufs.view(om, n * R, 1, 32)], 1)), terms=2)
    c0 = _plan.blind(engine, put(np.asarray(e, dtype=np.uint8).reshape(384)), s, messages, n)
    return bufs.view(c0, n, 384), bufs.view(c1, n, R, 384), bufs.view(c2, n, R, 128), bufs.view(c3, n, R, 128)


def encrypt_batch_seeded(engine, e, egg_alpha, g2_y, matrix, rho, messages, rng, table=None):
    """encrypt_batch with its randomness drawn on the device: rng is an rng.Randomness over the engine, everything else as there, and
    the return value is exactly encrypt_batch's on the scalars drawn.  The draws, in this order (the order is part of the interface: it
    is what makes the ciphertexts reproducible from the seed): s [n], v [n, C - 1], w [n, C - 1], r [n, R] — four stream ids, two when
    C == 1 (a draw of no columns takes none), none when n == 0.  The scalars are of the kind of `messages`.  The seed is key material:
    whoever holds it can recompute s and with it every message."""
    R, C = len(matrix), len(matrix[0]) if len(matrix) else 0
    n = bufs.nbytes(messages) // 384
    s = rng.scalars(messages, n)
    v = rng.scalars(messages, n, C - 1) if C > 1 else None
    w = rng.scalars(messages, n, C - 1) if C > 1 else None
    r = rng.scalars(messages, n, R)
    return encrypt_batch(engine, e, egg_alpha, g2_y, matrix, rho, messages, s, v, w, r, table=table)
