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

Host orchestration only, engine-agnostic (every function takes the engine: `bn254`, or a stand-in with the same function names).
Host arrays in give host arrays out; CUDA tensors in give CUDA tensors out, with only the key, the padded matrices, the mask and
an index table going to the device."""
import collections

import numpy as np

from . import _buffers as bufs
from ._buffers import R_ORDER
from .lw11 import reconstruction_weights

Padded = collections.namedtuple("Padded", "matrix rho rows cols")      # matrix [n, R, C, 32] uint8 scalars; rho [n, R] int64, -1 = padding
NO_ATTRIBUTE = -1


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
                one[:r, :c] = np.frombuffer(b"".join((int(v) % R_ORDER).to_bytes(32, "little") for row in m for v in row), dtype=np.uint8).reshape(r, c, 32)
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
    return engine.g1_multi_scalar_mul(bufs.flat(cx), bufs.flat(nw), np.arange(0, n * R + 1, R, dtype=np.uint64))


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
    E = engine.multi_pair(bufs.flat(P), bufs.flat(Q), np.arange(0, (R + 2) * n + 1, R + 2, dtype=np.uint64))
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
                for x, wx in zip(*got):
                    w[t, x] = np.frombuffer(int(wx).to_bytes(32, "little"), dtype=np.uint8)
        return put(w), put(ok)
    return _decrypt(engine, key, pad, c, c_prime, cx, dx, weights)
