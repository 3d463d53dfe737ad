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

Host orchestration only, engine-agnostic (every function takes the engine: `bn254`, or a stand-in with the same function names):
the elimination is per policy, microseconds in Python integers, and stays on the host."""
import numpy as np

from . import _buffers as bufs
from ._buffers import R_ORDER


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
    E = engine.multi_pair(bufs.flat(P), bufs.flat(Q), np.arange(0, 2 * k * n + 1, 2 * k, dtype=np.uint64))
    F = engine.gt_multi_exp(bufs.flat(used(c1, 384)), weights, np.arange(0, k * n + 1, k, dtype=np.uint64))
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
    table = np.arange(0, k * n + 1, k, dtype=np.uint64)
    S = engine.g2_multi_scalar_mul(bufs.flat(used(c3, 128)), weights, table).reshape(n, 1, 128)
    hb = np.concatenate([np.asarray(h_gid, dtype=np.uint8).reshape(1, 64), B])
    P = bufs.expand(bufs.put(hb.reshape(1, k + 1, 64), c0), n, k + 1, 64)
    Q = bufs.cat([S, used(c2, 128)], 1)
    E = engine.multi_pair(bufs.flat(P), bufs.flat(Q), np.arange(0, (k + 1) * n + 1, k + 1, dtype=np.uint64))
    F = engine.gt_multi_exp(bufs.flat(used(c1, 384)), weights, table)
    return engine.gt_div(bufs.flat(c0).reshape(n, 384), engine.gt_mul(E, F))
