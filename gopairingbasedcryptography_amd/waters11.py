"""Host-side planner for batched Waters 2011 ciphertext-policy ABE decryption (cpabe/waters11/waters11_cpabe.go:248-290): one user key
against a batch of ciphertexts, each under a policy of its own.

What is computed.  A ciphertext carries its LSSS policy (M, rho), so a batch against one key is a batch of different matrices.  With
the rows x whose attribute rho(x) the key holds and weights w_x such that sum_x w_x M_x = (1, 0, ..., 0),

    M = c / ( e(K, C') / prod_x ( e(C_x, L) e(K_rho(x), D_x) )^w_x )

because e(C_x, L) e(K_rho(x), D_x) = e(g1, g2)^(a t lambda_x) and the shares recombine to sum w_x lambda_x = s.  The exponents fold in
front of the pairings exactly — e(P, Q)^k = e([k] P, Q) as Fp12 elements, the argument lw11.py and sw05.py make — and the pairings
against the one L fold into one: prod_x e(C_x, L)^-w_x = e(S, L), S = sum_x [-w_x] C_x.  Per ciphertext

    E = Pair([K, S, T_x ...], [C', L, D_x ...]),  T_x = [-w_x] K_rho(x)        one multi-pairing segment of R + 2 pairs
    M = c / E

The weights differ from ciphertext to ciphertext, so unlike lw11.py (one policy for the whole batch, one elimination in host
integers) they are per item: engine.fr_lsss_weights solves the n systems on the device, and the weights go into engine.fr_neg and
engine.g1_scalar_mul (with msm=True: into engine.g1_multi_scalar_mul for S) as they are.  A row whose attribute the key lacks, a
dependent row and a padding row get weight 0, hence the point at infinity, which the group law and the pairing treat as gnark does
(e(0, Q) = 1).

The reference's loop is not quite that formula: it indexes the COMPACTED weight slice by the matrix row number (wSlice[i],
waters11_cpabe.go:280; SURVEY.md's notes on Waters11 / DABE), which agrees with the scheme only when the used rows are the first
rows of the matrix or all weights are equal.  This planner follows the scheme, as lw11.py does.  The weights themselves are the
ones of the greedy first basis of the held rows (include/gpbc_bn254.h), not necessarily the solution the reference's
back-substitution lands on: any valid weights give the same message.

Policies written as boolean formulas (formula.py) need neither the solve nor the multiplications: the matrix of a formula recombines
with weights 0 and 1, and decrypt_batch_formulas takes the rows with weight 1 from engine.formula_select (opt-in; decrypt_batch is
unchanged and takes formula.padded(...) like any other block).

Host orchestration only, engine-agnostic (every function takes the engine: `bn254`, or a stand-in with the same function names).
Host arrays in give host arrays out; CUDA tensors in give CUDA tensors out, with only the key, the padded matrices, the mask and
an index table going to the device.

Below Decrypt: Encrypt and KeyGenerate (:130-237), and at the end SetUp (:82-118) with the universe constructor of
waters11_cpabe_utils.go:29-41."""
import collections

import numpy as np

from . import _buffers as bufs, _plan
from ._plan import INDEX_NONE, NO_ATTRIBUTE      # noqa: F401 (INDEX_NONE: for callers that build index rows themselves)
from .lw11 import reconstruction_weights
from .sw05 import _power_of_pairing

Padded = collections.namedtuple("Padded", "matrix rho rows cols")      # matrix [n, R, C, 32] uint8 scalars; rho [n, R] int64, -1 = padding


def pad_policies(policies, rows=None, cols=None):
    """ragged (matrix, rho) pairs -> Padded: one [n, R, C] block of scalars (R, C = the largest row and column counts, or the ones
    given) and the [n, R] attribute table.  A padded row is all zero and carries NO_ATTRIBUTE, so it is never held; a padded column
    is all zero, an equation 0 = 0.  Attributes are integers in [0, 2^63).  A matrix object that occurs again is converted once."""
    n = len(policies)
    R = max([len(m) for m, _ in policies] + [1]) if rows is None else int(rows)
    C = max([len(m[0]) for m, _ in policies if len(m)] + [1]) if cols is None else int(cols)
    block = np.zeros((n, R, C, 32), dtype=np.uint8)
    table = np.full((n, R), NO_ATTRIBUTE, dtype=np.int64)
    done = {}
    for t, (m, rho) in enumerate(policies):
        key = (id(m), id(rho))
        if key not in done:
            r, c = len(m), len(m[0]) if len(m) else 0
            if r > R or c > C or len(rho) != r or any(len(row) != c for row in m):
                raise ValueError("policy %d: %d rows x %d columns with %d attributes does not fit [%d, %d]" % (t, r, c, len(rho), R, C))
            if any(not 0 <= int(a) < 1 << 63 for a in rho):
                raise ValueError("policy %d: attributes must be integers in [0, 2^63)" % t)
            one = np.zeros((R, C, 32), dtype=np.uint8)
            if r and c:
                one[:r, :c] = _plan.scalar_rows(v for row in m for v in row).reshape(r, c, 32)
            att = np.full(R, NO_ATTRIBUTE, dtype=np.int64)
            att[:r] = [int(a) for a in rho]
            done[key] = (one, att)
        block[t], table[t] = done[key]
    return Padded(block, table, R, C)


def _key_table(key_attrs):
    attrs = np.array(sorted(int(a) for a in key_attrs), dtype=np.int64)
    if attrs.size and (attrs[0] < 0 or (np.diff(attrs) == 0).any()):
        raise ValueError("key attributes must be distinct integers in [0, 2^63)")
    return attrs


def key_index(rho_table, key_attrs):
    """[n, R] int64: the position of rho[t][x] in sorted(key_attrs), len(key_attrs) where the key lacks it (and for padding)"""
    attrs = _key_table(key_attrs)
    rho = np.asarray(rho_table, dtype=np.int64)
    if not attrs.size:
        return np.zeros(rho.shape, dtype=np.int64)
    pos = np.minimum(np.searchsorted(attrs, rho), attrs.size - 1)
    return np.where(attrs[pos] == rho, pos, attrs.size)


def held_mask(rho_table, key_attrs):
    """[n, R] uint8: 1 where the key holds rho[t][x] (numpy, no loop over the ciphertexts)"""
    return (key_index(rho_table, key_attrs) < len(key_attrs)).astype(np.uint8)


def _row_sums_composed(engine, cx, nw, n, R):
    """S_t = sum_x [-w_tx] C_tx: n R scalar multiplications, then ceil(log2 R) rounds of additions over the row axis"""
    S = engine.g1_scalar_mul(bufs.flat(cx), bufs.flat(nw)).reshape(n, R, 64)
    m = R
    while m > 1:
        h = m // 2
        s = engine.g1_add(bufs.flat(S[:, :h]), bufs.flat(S[:, h:2 * h])).reshape(n, h, 64)
        S = bufs.cat([s, S[:, 2 * h:m]], 1) if m & 1 else s
        m = h + (m & 1)
    return S


def _row_sums_msm(engine, cx, nw, n, R):
    """the same sums from one segmented multi-scalar multiplication: n segments of R terms, the doublings shared by four terms"""
    return engine.g1_multi_scalar_mul(bufs.flat(cx), bufs.flat(nw), _plan.segments(n, R))


def _decrypt(engine, key, pad, c, c_prime, cx, dx, weights, row_sums=_row_sums_composed):
    K, L, kx = key
    n, R = pad.rho.shape
    bufs.device_of(c, c_prime, cx, dx)                                         # all of one kind, on one device
    if bufs.nbytes(c) != n * 384 or bufs.nbytes(c_prime) != n * 128 or bufs.nbytes(cx) != n * R * 64 or bufs.nbytes(dx) != n * R * 128:
        raise ValueError("need c [n, 384], c_prime [n, 128], cx [n, R, 64], dx [n, R, 128] with n = %d, R = %d" % (n, R))

    def put(a):
        return bufs.put(a, c)
    c, c_prime, cx, dx = bufs.view(c, n, 384), bufs.view(c_prime, n, 1, 128), bufs.view(cx, n * R, 64), bufs.view(dx, n, R, 128)
    if not n:
        return bufs.zeros((0, 384), c), bufs.zeros((0,), c)
    attrs = sorted(int(a) for a in kx)
    comp = np.zeros((len(attrs) + 1, 64), dtype=np.uint8)                 # the last row: the point at infinity, for rows the key lacks
    for i, a in enumerate(attrs):
        comp[i] = np.asarray(kx[a], dtype=np.uint8).reshape(64)
    index = key_index(pad.rho, attrs)
    held = (index < len(attrs)).astype(np.uint8)
    w, ok = weights(put, held)                                                # [n, R, 32] canonical, [n]
    nw = engine.fr_neg(bufs.flat(w))
    S = row_sums(engine, cx, nw, n, R)
    # T_tx = [-w_tx] K_rho(t,x)
    gathered = bufs.take(put(comp), index.reshape(-1))
    T = engine.g1_scalar_mul(bufs.flat(gathered), bufs.flat(nw)).reshape(n, R, 64)
    k_rows = put(np.broadcast_to(np.asarray(K, dtype=np.uint8).reshape(1, 1, 64), (n, 1, 64)))
    l_rows = put(np.broadcast_to(np.asarray(L, dtype=np.uint8).reshape(1, 1, 128), (n, 1, 128)))
    P = bufs.cat([k_rows, S.reshape(n, 1, 64), T], 1)
    Q = bufs.cat([c_prime, l_rows, dx], 1)
    E = engine.multi_pair(bufs.flat(P), bufs.flat(Q), _plan.segments(n, R + 2))
    msgs = engine.gt_div(bufs.flat(c), bufs.flat(E)).reshape(n, 384)
    ok = ok.reshape(n)
    return msgs * ok.reshape(n, 1), ok                                         # ok is 0 / 1: a row that cannot be decrypted comes back all zero


def decrypt_batch(engine, key, policies_or_padded, c, c_prime, cx, dx, msm=False):
    """The n messages of n ciphertexts, each under its own policy, for one key.  key = (K [64], L [128], kx: attribute -> [64]) as
    host bytes; policies_or_padded: n (matrix, rho) pairs or the Padded block of pad_policies; c [n, 384], c_prime [n, 128],
    cx [n, R, 64], dx [n, R, 128] with R the padded row count (rows past a policy's own may hold anything: their weight is 0).
    Returns (messages [n, 384], ok [n]); a ciphertext whose policy the key does not satisfy has ok = 0 and an all-zero row.
    Engine calls: fr_lsss_weights (a matrix per ciphertext), fr_neg, g1_scalar_mul twice over n R points with the device scalars,
    ceil(log2 R) rounds of g1_add, multi_pair with one segment of R + 2 pairs per ciphertext, gt_div.  With msm=True the first
    g1_scalar_mul and the rounds of g1_add are ONE g1_multi_scalar_mul (n segments of R terms); the messages are the same bytes."""
    pad = policies_or_padded if isinstance(policies_or_padded, Padded) else pad_policies(policies_or_padded)

    def weights(put, held):
        return engine.fr_lsss_weights(put(pad.matrix).reshape(-1), pad.rows, pad.cols, put(held).reshape(-1))
    return _decrypt(engine, key, pad, c, c_prime, cx, dx, weights, _row_sums_msm if msm else _row_sums_composed)


def decrypt_batch_host_weights(engine, key, policies, c, c_prime, cx, dx):
    """decrypt_batch with the weights from lw11.reconstruction_weights, one elimination in Python integers per ciphertext: the route
    the engine had before fr_lsss_weights.  For the comparison and the tests only; policies are the (matrix, rho) pairs."""
    pad = pad_policies(policies)
    attrs = set(int(a) for a in key[2])

    def weights(put, held):
        n, R = pad.rho.shape
        w, ok = np.zeros((n, R, 32), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        for t, (m, rho) in enumerate(policies):
            got = reconstruction_weights(m, rho, attrs) if len(m) else None
            if got is not None:
                ok[t] = 1
                w[t, got[0]] = _plan.scalar_rows(got[1])
        return put(w), put(ok)
    return _decrypt(engine, key, pad, c, c_prime, cx, dx, weights)


def decrypt_batch_formulas(engine, key, nodes, c, c_prime, cx, dx, rows=None):
    """decrypt_batch for ciphertexts whose policies are boolean formulas (formula.encode: [n, N] int64 codes, a host array or a tensor
    where the ciphertexts are), encrypted under formula.padded(...).  The matrix of a formula recombines with weights 0 and 1: the
    leaves engine.formula_select reaches from a satisfied root.  So no system is solved and no point is multiplied:

        S = -(sum of the chosen C_x),  T_x = -K_rho(x) for the chosen rows, the point at infinity elsewhere,

    in front of the same multi-pairing segments of R + 2 pairs and gt_div.  rows: R of cx and dx (None: the largest leaf count).
    Returns (messages [n, 384], ok [n]), byte for byte those of decrypt_batch on formula.padded(...): GT output is canonical and any
    valid weights give the same message.  An unsatisfied or malformed formula has ok = 0 and an all-zero row.  Engine calls:
    formula_select, g1_sum_segments (n segments of R points), g1_sub twice (the n sums and the key's components from infinity),
    multi_pair, gt_div."""
    from . import formula
    K, L, kx = key
    rho = formula.leaves(nodes, rows, strict=False)
    n, R = rho.shape
    bufs.device_of(c, c_prime, cx, dx)                                         # all of one kind, on one device
    if bufs.nbytes(c) != n * 384 or bufs.nbytes(c_prime) != n * 128 or bufs.nbytes(cx) != n * R * 64 or bufs.nbytes(dx) != n * R * 128:
        raise ValueError("need c [n, 384], c_prime [n, 128], cx [n, R, 64], dx [n, R, 128] with n = %d, R = %d" % (n, R))

    def put(a):
        return bufs.put(a, c)
    c, c_prime, cx, dx = bufs.view(c, n, 384), bufs.view(c_prime, n, 1, 128), bufs.view(cx, n * R, 64), bufs.view(dx, n, R, 128)
    if not n:
        return bufs.zeros((0, 384), c), bufs.zeros((0,), c)
    attrs = sorted(int(a) for a in kx)
    comp = np.zeros((len(attrs) + 1, 64), dtype=np.uint8)                 # the last row: the point at infinity, for rows the key lacks
    for i, a in enumerate(attrs):
        comp[i] = np.asarray(kx[a], dtype=np.uint8).reshape(64)
    index = key_index(rho, attrs)
    held = (index < len(attrs)).astype(np.uint8)
    codes = nodes if bufs.is_torch(nodes) else put(np.ascontiguousarray(nodes, dtype=np.int64))
    chosen, ok = engine.formula_select(codes, put(held).reshape(-1), R)        # [n, R] of 0 / 1, [n]
    chosen = bufs.view(chosen, n * R, 1)
    sums = engine.g1_sum_segments(bufs.flat(cx * chosen), _plan.segments(n, R))
    S = engine.g1_sub(bufs.flat(bufs.zeros((n, 64), c)), bufs.flat(sums))
    neg = engine.g1_sub(bufs.flat(bufs.zeros((len(attrs) + 1, 64), c)), bufs.flat(put(comp)))
    T = (bufs.take(bufs.view(neg, len(attrs) + 1, 64), index.reshape(-1)) * chosen).reshape(n, R, 64)
    k_rows = put(np.broadcast_to(np.asarray(K, dtype=np.uint8).reshape(1, 1, 64), (n, 1, 64)))
    l_rows = put(np.broadcast_to(np.asarray(L, dtype=np.uint8).reshape(1, 1, 128), (n, 1, 128)))
    P = bufs.cat([k_rows, bufs.view(S, n, 1, 64), T], 1)
    Q = bufs.cat([c_prime, l_rows, dx], 1)
    E = engine.multi_pair(bufs.flat(P), bufs.flat(Q), _plan.segments(n, R + 2))
    msgs = engine.gt_div(bufs.flat(c), bufs.flat(E)).reshape(n, 384)
    ok = ok.reshape(n)
    return msgs * ok.reshape(n, 1), ok


# ------------------------------------------------------------------------------------------------ Encrypt and KeyGenerate
# cpabe/waters11/waters11_cpabe.go:82-237.  Every base of the two loops is a public parameter — g1^a and the h_u of the universe — so
# they are sums over ONE fixed-base table (engine.FixedBase.indexed): base 0 is g1^a, base 1 + i the h of the i-th attribute in
# ascending order.  The shares are engine.fr_lsss_shares on the padded matrices as decrypt_batch takes them.  The randomness is passed
# in, as in bsw07.encrypt_batch.
def _universe(h):
    attrs = sorted(int(u) for u in h)
    if any(a < 0 for a in attrs):
        raise ValueError("attributes must be integers in [0, 2^63)")
    return attrs


def encrypt_table(engine, g1a, h):
    """The fixed-base table of encrypt_batch and keygen_batch over (g1^a, h_u ...), h_u in ascending order of u: built once, passed
    as `table` to any number of calls, closed by the caller (table.close())."""
    attrs = _universe(h)
    bases = np.stack([np.asarray(g1a, dtype=np.uint8).reshape(64)] + [np.asarray(h[u], dtype=np.uint8).reshape(64) for u in attrs])
    return engine.FixedBase(bases, g2=False)


def _attribute_positions(table_attrs, wanted, what):
    """1 + position in the universe per wanted attribute (base 0 is g1^a); NO_ATTRIBUTE stays NO_ATTRIBUTE.  An attribute outside the
    universe is the reference's checkAttributes error."""
    univ = np.array(table_attrs, dtype=np.int64)
    wanted = np.asarray(wanted, dtype=np.int64)
    real = wanted != NO_ATTRIBUTE
    if real.any() and not univ.size:
        raise ValueError("%s: attribute %d is not in the universe" % (what, int(wanted[real][0])))
    pos = np.minimum(np.searchsorted(univ, wanted), max(univ.size - 1, 0))
    miss = real & (univ[pos] != wanted if univ.size else real)
    if miss.any():
        raise ValueError("%s: attribute %d is not in the universe" % (what, int(wanted[miss][0])))
    return np.where(real, pos + 1, NO_ATTRIBUTE)


def _table(engine, table, g1a, h, attrs):
    """the caller's table, or encrypt_table's for this call alone; either way over g1^a and the whole universe"""
    return _plan.handle(table, lambda: encrypt_table(engine, g1a, h), "nbase", 1 + len(attrs), "the table holds %(got)d bases, the universe needs %(want)d")


def encrypt_batch(engine, g1a, e_alpha, h, policies_or_padded, messages, s, v, r, table=None):
    """n ciphertexts, each under a policy of its own (Encrypt, waters11_cpabe.go:170-237).  g1a = g1^a (64 B) and e_alpha =
    e(g1, g2)^alpha (384 B) of the public key; h: {attribute: 64-byte G1 point}, the universe; policies_or_padded: n (matrix, rho) pairs
    or pad_policies' block [n, R, C]; messages [n, 384]; s: n scalars; v: [n, C - 1] scalars, the rest of the share vector (s, v_2, ..);
    r: [n, R] scalars, r_x of every row.  Scalars are Python ints, uint8 arrays or CUDA tensors.

    The shares are taken over every ROW of the matrix, lambda_x = M_x . (s, v), as the scheme and decrypt_batch have it; the reference's
    loop runs to ColumnNumber() (waters11_cpabe.go:182,211), which covers every row only for a square matrix.

    Returns exactly the operands of decrypt_batch: (c [n, 384], c_prime [n, 128], cx [n, R, 64], dx [n, R, 128]) with
    C_x = [lambda_x] g1^a + [-r_x] h_rho(x), D_x = [r_x] g2, C' = [s] g2, C = M e(g1, g2)^(alpha s).  A padding row (zero matrix row,
    attribute -1) gets the index (0, none), so its C_x is the point at infinity; its D_x is [r_x] g2 like any other.  An attribute of a
    policy that is not in h is a ValueError (checkAttributes).  table: encrypt_table(engine, g1a, h) built once by the caller; None
    builds and closes one here.  Engine calls: fr_lsss_shares (a matrix per ciphertext), fr_neg, FixedBase.indexed (terms = 2, an index
    row per output), g2_scalar_mul_base twice, gt_exp, gt_mul."""
    pad = policies_or_padded if isinstance(policies_or_padded, Padded) else pad_policies(policies_or_padded)
    n, R = pad.rho.shape
    C = pad.cols
    attrs = _universe(h)
    pos = _attribute_positions(attrs, pad.rho, "policy")                      # before anything touches the engine
    if bufs.nbytes(messages) != n * 384:
        raise ValueError("messages must hold n = %d GT elements" % n)
    s, v, r = _plan.scalars(s, messages), (None if v is None else _plan.scalars(v, messages)), _plan.scalars(r, messages)
    bufs.device_of(messages, s, v, r)                                          # all of one kind, on one device
    if bufs.nbytes(s) != n * 32 or (bufs.nbytes(v) if v is not None else 0) != n * (C - 1) * 32 or bufs.nbytes(r) != n * R * 32:
        raise ValueError("need s [n], v [n, C - 1], r [n, R] scalars with n = %d, R = %d, C = %d" % (n, R, C))
    if not n:
        return bufs.zeros((0, 384), messages), bufs.zeros((0, 128), messages), bufs.zeros((0, R, 64), messages), bufs.zeros((0, R, 128), messages)
    s, r = bufs.view(s, n, 1, 32), bufs.view(r, n * R, 1, 32)
    vec = s if C == 1 else bufs.cat([s, bufs.view(v, n, C - 1, 32)], 1)
    lam = engine.fr_lsss_shares(bufs.flat(bufs.put(pad.matrix, messages)), bufs.flat(vec), pad.rows, pad.cols)        # [n, R, 32]
    nr = engine.fr_neg(bufs.flat(r))
    index = np.stack([np.zeros(n * R, dtype=np.int64), pos.reshape(-1)], 1)                                           # (g1^a, h_rho(x)); padding: (g1^a, none)
    with _table(engine, table, g1a, h, attrs) as table:
        scal = bufs.cat([bufs.view(lam, n * R, 1, 32), bufs.view(nr, n * R, 1, 32)], 1)
        cx, ok = table.indexed(_plan.index_rows(index, messages), bufs.flat(scal), terms=2)
    dx = engine.g2_scalar_mul_base(bufs.flat(r))
    c_prime = engine.g2_scalar_mul_base(bufs.flat(s))
    c = _plan.blind(engine, _plan.public(e_alpha, 1, 384, messages, "e_alpha"), s, messages, n)
    return bufs.view(c, n, 384), bufs.view(c_prime, n, 128), bufs.view(cx, n, R, 64), bufs.view(dx, n, R, 128)


def encrypt_batch_seeded(engine, g1a, e_alpha, h, policies_or_padded, messages, rng, table=None):
    """encrypt_batch with its randomness drawn on the device: rng is an rng.Randomness over the engine, everything else as there, and
    the return value is exactly encrypt_batch's on the scalars drawn.  The draws, in this order (the order is part of the interface: it
    is what makes the ciphertexts reproducible from the seed): s [n], v [n, C - 1], r [n, R], with R and C the padded block's common
    shape — three stream ids, two when C == 1 (a draw of no columns takes none), none when n == 0.  The scalars are of the kind of
    `messages`.  The seed is key material: whoever holds it can recompute s and with it every message."""
    pad = policies_or_padded if isinstance(policies_or_padded, Padded) else pad_policies(policies_or_padded)
    n, R = pad.rho.shape
    s = rng.scalars(messages, n)
    v = rng.scalars(messages, n, pad.cols - 1) if pad.cols > 1 else None
    r = rng.scalars(messages, n, R)
    return encrypt_batch(engine, g1a, e_alpha, h, pad, messages, s, v, r, table=table)


def keygen_batch(engine, g1_alpha, g1a, h, user_attrs, t, table=None):
    """Keys of n users (KeyGenerate, waters11_cpabe.go:130-168): K = g1^alpha + [t] g1^a, L = [t] g2, K_x = [t] h_x for the user's
    attributes.  g1_alpha = g1^alpha (64 B, the master key), g1a and h as in encrypt_batch; user_attrs: n lists of attributes, each
    within the universe (ValueError otherwise: checkAttributes) and without repeats; t: n scalars.  Returns (K [n, 64], L [n, 128],
    kx [n, A, 64], attrs [n, A] int64) with A the largest attribute count: a user's attributes in ascending order, then NO_ATTRIBUTE
    with the point at infinity.  (K[j], L[j], {attrs[j][i]: kx[j][i]}) is the key decrypt_batch takes.  Engine calls:
    FixedBase.indexed (terms = 1, 1 + A outputs per user), g1_add, g2_scalar_mul_base."""
    attrs = _universe(h)
    users = [sorted(int(a) for a in ua) for ua in user_attrs]
    n = len(users)
    if any(len(set(u)) != len(u) for u in users):
        raise ValueError("a user's attributes must be distinct")
    A = max([len(u) for u in users] + [1])
    held = np.full((n, A), NO_ATTRIBUTE, dtype=np.int64)
    for j, u in enumerate(users):
        held[j, :len(u)] = u
    pos = _attribute_positions(attrs, held, "user")
    like = t if bufs.is_torch(t) else np.zeros(0, dtype=np.uint8)
    t = _plan.scalars(t, like)
    if bufs.nbytes(t) != n * 32:
        raise ValueError("t must hold n = %d scalars" % n)
    if not n:
        return bufs.zeros((0, 64), t), bufs.zeros((0, 128), t), bufs.zeros((0, A, 64), t), held
    t = bufs.view(t, n, 1, 32)
    index = np.concatenate([np.zeros((n, 1), dtype=np.int64), pos], 1).reshape(-1, 1)                                 # [t] g1^a, then [t] h_x
    with _table(engine, table, g1a, h, attrs) as table:
        pts, ok = table.indexed(_plan.index_rows(index, t), bufs.flat(bufs.expand(t, n, 1 + A, 32)), terms=1)
    pts = bufs.view(pts, n, 1 + A, 64)
    K = engine.g1_add(bufs.flat(bufs.expand(_plan.public(g1_alpha, 1, 64, t, "g1_alpha"), n, 64)), bufs.flat(pts[:, 0]))
    L = engine.g2_scalar_mul_base(bufs.flat(t))
    return bufs.view(K, n, 64), bufs.view(L, n, 128), pts[:, 1:], held


# ------------------------------------------------------------------------------------------------ SetUp
# cpabe/waters11/waters11_cpabe.go:82-118 and waters11_cpabe_utils.go:29-41.  The universe is a list of distinct integers in [0, 2^63), as
# every function above takes attributes; the public parameters come back as host arrays — they are public, h is a dict of host rows in
# encrypt_table's and keygen_batch's form, and every function above puts them where its batch lives — and g1^alpha of the kind the
# secrets are.
def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def universe_range(start, end):
    """the attributes start .. end - 1 (NewWaters11CPABEInstanceByInt64Pair, waters11_cpabe_utils.go:29-41): end < start is a ValueError,
    as there; end == start is the empty universe, which setup accepts.  Attributes here are integers in [0, 2^63), so a negative start
    is refused where the reference would read it as r - |start|."""
    if not _is_int(start) or not _is_int(end):
        raise ValueError("start and end must be integers")
    start, end = int(start), int(end)
    if end < start:
        raise ValueError("end must be greater than start")
    if start < 0 or end > 1 << 63:
        raise ValueError("attributes must be integers in [0, 2^63)")
    return list(range(start, end))


def _setup_universe(universe):
    universe = list(universe)
    if not all(_is_int(u) for u in universe):                                  # no int(): 3.7 is not attribute 3, True not attribute 1
        raise ValueError("the universe must hold distinct integers in [0, 2^63)")
    attrs = sorted(int(u) for u in universe)
    if any(not 0 <= u < 1 << 63 for u in attrs) or len(set(attrs)) != len(attrs):
        raise ValueError("the universe must hold distinct integers in [0, 2^63)")
    return attrs


def setup(engine, universe, alpha, a, tau, gt_table=None):
    """(pp, msk) from the secrets (SetUp, waters11_cpabe.go:82-118): pp = {"g1a": [a] g1 (64 B), "e_alpha": e(g1, g2)^alpha (384 B),
    "h": {u: [tau_u] g1 (64 B)}} as host arrays — exactly the (g1a, e_alpha, h) arguments of encrypt_batch, keygen_batch and encrypt_table
    — and msk = {"g1_alpha": [alpha] g1 (64 B)}, keygen_batch's g1_alpha, of the kind the secrets are.  universe: distinct integers in
    [0, 2^63), in any order (universe_range makes one); alpha, a: one scalar each; tau: one scalar per attribute, tau[i] belonging to the
    i-th attribute in ASCENDING order, whatever order the universe was given in (Python ints, 32-byte rows or CUDA tensors, all of one
    kind).  The empty universe gives h = {}.  gt_table: an engine.GTFixedBase whose base 0 is e(g1, g2), built once by the caller;
    e_alpha then comes from its indexed products and is the same bytes.  Engine calls: ONE g1_scalar_mul_base over (a, alpha, tau ...);
    pair_batch on the generators and gt_exp, or gt_table.indexed with one term."""
    attrs = _setup_universe(universe)                                          # before anything touches the engine
    U = len(attrs)
    like = _plan.like_of(alpha, a, tau)
    alpha, a, tau = _plan.scalars(alpha, like, 1, "alpha"), _plan.scalars(a, like, 1, "a"), _plan.scalars(tau, like, U, "tau")
    bufs.device_of(alpha, a, tau)
    pts = bufs.view(engine.g1_scalar_mul_base(bufs.flat(bufs.cat([a, alpha, tau]))), 2 + U, 64)
    e_alpha = _power_of_pairing(engine, alpha, like, gt_table)
    host = np.array(_plan.host(pts), dtype=np.uint8, copy=True)
    pp = {"g1a": host[0], "e_alpha": np.array(_plan.host(e_alpha), dtype=np.uint8, copy=True).reshape(384), "h": {u: host[2 + i] for i, u in enumerate(attrs)}}
    return pp, {"g1_alpha": bufs.view(pts[1], 64)}


def setup_seeded(engine, universe, rng, like=None, gt_table=None):
    """setup with the secrets drawn on the device: rng is an rng.Randomness over the engine.  The draws, in this order (the order is part
    of the interface: it is what makes the keys reproducible from the seed): alpha, then a, then tau [U] — the reference's order
    (:84-107), three stream ids, two for an empty universe.  The reference draws tau_u while it ranges over a Go map, in an order that
    differs from run to run; here tau_u belongs to the u-th attribute in ascending order.  A refused universe draws nothing.  like: a
    buffer of the kind the master key is to be (None: a host array).  The seed is key material: whoever holds it holds the master key."""
    attrs = _setup_universe(universe)
    like = np.zeros(0, dtype=np.uint8) if like is None else like
    alpha = rng.scalars(like, 1)
    a = rng.scalars(like, 1)
    tau = rng.scalars(like, len(attrs))
    return setup(engine, attrs, alpha, a, tau, gt_table=gt_table)
