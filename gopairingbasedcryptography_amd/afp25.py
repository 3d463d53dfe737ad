"""Host-side planner for batched AFP25 batched-IBE decryption (BASELINE config 5).

Reference flow (bibe/afp25_bibe/afp25_bibe.go:369-418, afp25_bibe_utils.go:14-55): to decrypt for identity id inside a
batch of B identities, rebuild the quotient polynomial q(X) = f(X)/(X - id) by multiplying out B-1 linear factors
(O(B^2) Fr operations), commit to it with B separate G1 scalar multiplications and B affine additions, run THREE full
pairings e(D, C1[0]), e(pi, C1[1]), e(sk, C1[2]), multiply them and divide C2 by the product.

Batched form used here, bit-identical in its GT result:
  * f(X) is expanded once per batch; every q_i(X) comes from it by synthetic division (O(B) each);
  * pi_i = sum_j coef_j * [tau^j]_1 through the engine's G1 scalar-multiplication kernel and point-sum tree;
  * all items of the batch go through ONE multi_pair call (3 Miller loops + 1 final exponentiation per item) and one gt_div.
Host orchestration only; all group arithmetic goes through the engine (`bn254`).
"""
import numpy as np

from . import _buffers as bufs, _plan
from ._buffers import R_ORDER


def poly_from_roots(roots):
    """Coefficients (constant term first) of prod (X - root) mod r  (computePolynomialCoeffs, afp25_bibe_utils.go:14-43)."""
    coeffs = [1]
    for root in roots:
        new = [0] * (len(coeffs) + 1)
        for i, c in enumerate(coeffs):
            new[i] = (new[i] - root * c) % R_ORDER
            new[i + 1] = (new[i + 1] + c) % R_ORDER
        coeffs = new
    return coeffs


def quotient_by_root(coeffs, root):
    """f(X) / (X - root) by synthetic division; raises if root is not a root (identity not in the batch)."""
    n = len(coeffs) - 1
    q = [0] * n
    carry = 0
    for i in range(n, 0, -1):
        carry = (coeffs[i] + carry * root) % R_ORDER
        q[i - 1] = carry
    if (coeffs[0] + carry * root) % R_ORDER != 0:
        raise ValueError("identity not found in identity list")
    return q


def commit_g1(engine, g1, tau_powers, coeffs):
    """[p(tau)]_1 = coef_0*g1 + sum_j coef_j*[tau^j]_1  (computeG1PolynomialTau, afp25_bibe_utils.go:45-55)."""
    pts = np.concatenate([np.asarray(g1, dtype=np.uint8).reshape(1, 64), np.asarray(tau_powers, dtype=np.uint8)[: len(coeffs) - 1]])
    if hasattr(engine, "g1_scalar_mul_sum"):                    # one call: sum_j [c_j] srs_j (the bucket method from 16 384 terms on)
        return np.asarray(engine.g1_scalar_mul_sum(pts, [int(c) for c in coeffs]))
    return np.asarray(engine.g1_sum(engine.g1_scalar_mul(pts, [int(c) for c in coeffs])))


def digest(engine, g1, tau_powers, identities):
    """Batch digest D = [f(tau)]_1, f(X) = prod (X - id)  (Digest, afp25_bibe.go:293-305). Returns (D, f coefficients)."""
    if len(identities) == 0:
        raise ValueError("identities is empty")
    if len(identities) > len(tau_powers):
        raise ValueError("too many identities for batch size")
    f = poly_from_roots(identities)
    return commit_g1(engine, g1, tau_powers, f), f


def srs_table(engine, g1, tau_powers):
    """Fixed-base window tables (engine.FixedBase, HBM-resident) over the commitment bases (g1, [tau]_1, ..., [tau^B]_1):
    built once per SRS, after which every commitment is ONE row of a multi-scalar multiplication."""
    return engine.FixedBase(np.concatenate([np.asarray(g1, dtype=np.uint8).reshape(1, 64), np.asarray(tau_powers, dtype=np.uint8).reshape(-1, 64)]))


def commit_g1_many(table, coeff_rows):
    """[p_i(tau)]_1 for every coefficient row (lowest degree first; rows are zero-padded to the table's nbase)."""
    rows = [[int(c) for c in r] + [0] * (table.nbase - len(r)) for r in coeff_rows]
    return np.asarray(table.msm(rows))


def decrypt_batch(engine, g1, tau_powers, D, f_coeffs, sk, items, table=None, identities=None):
    """items: list of (identity, C1 [3,128], C2 [384]) all encrypted under the batch digest D and key sk.
    identities: the batch's identity list (what Digest was computed from); when given, the reference's error behaviour for
    absent and for duplicated identities is reproduced (a duplicated identity is still a root of f, so the quotient alone
    would not notice it).
    Returns the messages [n,384]: m_i = C2_i / (e(D, C1_i[0]) e(pi_i, C1_i[1]) e(sk, C1_i[2])).
    With `table` (srs_table) all opening proofs pi_i come from one fixed-base MSM call instead of one scalar-multiplication
    batch and one point sum per item."""
    if identities is not None:
        # the reference's Decrypt removes every identity equal to id from the batch list and fails unless exactly one was
        # removed (bibe/afp25_bibe/afp25_bibe.go:371-381): an identity that is absent OR duplicated in the batch is an error
        for ident, _, _ in items:
            if sum(1 for x in identities if x % R_ORDER == ident % R_ORDER) != 1:
                raise ValueError("identity not found in identity list")
    if table is not None:
        pis = commit_g1_many(table, [quotient_by_root(f_coeffs, ident) for ident, _, _ in items])
    else:
        pis = [commit_g1(engine, g1, tau_powers, quotient_by_root(f_coeffs, ident)) for ident, _, _ in items]
    P_rows, Q_rows, c2 = [], [], []
    for (ident, C1, C2), pi in zip(items, pis):
        P_rows.append(np.stack([np.asarray(D, dtype=np.uint8), np.asarray(pi, dtype=np.uint8).reshape(64), np.asarray(sk, dtype=np.uint8)]))
        Q_rows.append(np.asarray(C1, dtype=np.uint8).reshape(3, 128))
        c2.append(np.asarray(C2, dtype=np.uint8))
    X = engine.multi_pair(np.concatenate(P_rows), np.concatenate(Q_rows), _plan.segments(len(items), 3))
    return engine.gt_div(np.stack(c2), X)


def decrypt_batch_arrays(engine, D, pi, sk, C1, C2):
    """The pairing part of the batch decryption on arrays (numpy, or CUDA tensors): item i is decrypted with its batch's
    digest D[i], its opening proof pi[i] and key sk[i] — m_i = C2_i / (e(D_i, C1_i[0]) e(pi_i, C1_i[1]) e(sk_i, C1_i[2]))
    (bibe/afp25_bibe/afp25_bibe.go:395-413): ONE multi-pairing of 3-pair segments and one gt_div, BASELINE config 5 at its
    stated size.  D, pi, sk: [n,64]; C1: [n,3,128]; C2: [n,384]."""
    n = bufs.nbytes(D) // 64
    P = bufs.cat([bufs.view(D, n, 1, 64), bufs.view(pi, n, 1, 64), bufs.view(sk, n, 1, 64)], 1)
    X = engine.multi_pair(bufs.flat(P), bufs.flat(bufs.view(C1, 3 * n, 128)), _plan.segments(n, 3))
    return engine.gt_div(bufs.flat(C2).reshape(n, 384), X)


# ----------------------------------------------------------------------------------------------- from identities and SRS
# The same decryption with the scalar work on the device (engine.fr_poly_from_roots / fr_poly_quotients, csrc/gpbc_fr.hip): a batch's
# f(X) is one workgroup, every quotient f(X) / (X - id) one lane, and the coefficient rows go straight from the kernel that makes them
# into the fixed-base MSM over the SRS table (srs_table: g1, [tau]_1 ... [tau^B]_1) as its scalars.  With CUDA tensors nothing but
# the identities going in and the messages coming out crosses PCIe.  The functions above stay as the host statement of the same
# computation; tests compare the two bit for bit.
QUOTIENT_SCRATCH_BYTES = 256 << 20      # bound on the quotient rows held at once (k x B x (B + 1) x 32 bytes in all: 2.2 GB at 1024 x 256)


def _identity_rows(engine, table, ids):
    """ids -> (flat scalar rows, k, B) with B = table.nbase - 1: [k][B] Python integers (host rows; the reference's rule that an
    identity occurs exactly once in its batch, afp25_bibe.go:371-381, is checked here), or k*B scalar rows as a uint8 array / CUDA
    tensor (taken as they are: keeping a batch's identities distinct is then the caller's business)."""
    B = table.nbase - 1
    if B < 1:
        raise ValueError("the SRS table needs at least two bases (g1 and [tau]_1)")
    if bufs.is_torch(ids) or isinstance(ids, np.ndarray) and ids.dtype == np.uint8:
        flat = ids.reshape(-1)
        size = bufs.nbytes(flat)
        if size % 32 or size == 0 or (size // 32) % B:
            raise ValueError("ids must hold a whole number of batches of B = %d identities (32 bytes each)" % B)
        return flat, size // 32 // B, B
    rows = [[int(x) for x in r] for r in ids]
    if not rows or any(len(r) != B for r in rows):
        raise ValueError("ids must hold a whole number of batches of B = %d identities" % B)
    for r in rows:
        if len({x % R_ORDER for x in r}) != B:
            raise ValueError("identity not found in identity list")          # duplicated in its batch: the reference removes more than one
    return engine.fr_to_bytes([x for r in rows for x in r]), len(rows), B


def digests(engine, table, ids):
    """D_j = [f_j(tau)]_1, f_j(X) = prod_i (X - ids[j][i]), for k batches (Digest, afp25_bibe.go:293-305): [k, 64].
    One kernel expands all f_j, one fixed-base MSM row per batch commits to them."""
    rows, k, B = _identity_rows(engine, table, ids)
    return table.msm(engine.fr_poly_from_roots(rows, B).reshape(-1))


def opening_proofs(engine, table, ids, coeffs=None):
    """pi[j*B + i] = [f_j(tau) / (tau - ids[j][i])]_1 for every identity of every batch: [k*B, 64].  coeffs: the f_j as
    fr_poly_from_roots gives them (computed here when None).  The quotient rows (B + 1 scalars each) are made chunk by chunk of
    whole batches in ONE scratch buffer of at most QUOTIENT_SCRATCH_BYTES and consumed by the MSM before the next chunk overwrites
    them.  An identity that is not a root of its batch's polynomial raises ValueError, as quotient_by_root does."""
    rows, k, B = _identity_rows(engine, table, ids)
    stride = table.nbase
    if coeffs is None:
        coeffs = engine.fr_poly_from_roots(rows, B)
    coeffs = coeffs.reshape(-1)
    per_batch = B * stride * 32
    chunk = min(k, max(1, QUOTIENT_SCRATCH_BYTES // per_batch))
    scratch, okbuf, pi = bufs.empty((chunk * per_batch,), rows), bufs.empty((chunk * B,), rows), bufs.empty((k * B, 64), rows)
    for lo in range(0, k, chunk):
        m = min(chunk, k - lo)
        q, ok = engine.fr_poly_quotients(coeffs[lo * (B + 1) * 32:(lo + m) * (B + 1) * 32], rows[lo * B * 32:(lo + m) * B * 32], B, stride,
                                         out=scratch[:m * per_batch], ok=okbuf[:m * B])
        pi[lo * B:(lo + m) * B] = table.msm(q)
        if not bool(ok.all()):
            raise ValueError("identity not found in identity list")
    return pi


def decrypt_batches(engine, table, ids, sk, C1, C2, D=None):
    """Decrypt k batches of B items from their identities and the SRS table: digests (unless D is given), opening proofs, then
    decrypt_batch_arrays.  ids: as _identity_rows takes them; sk, D: [k, 64] (one per batch) or [k*B, 64] (one per item);
    C1: [k*B, 3, 128]; C2: [k*B, 384].  Returns the messages [k*B, 384]."""
    rows, k, B = _identity_rows(engine, table, ids)
    coeffs = engine.fr_poly_from_roots(rows, B)
    if D is None:
        D = table.msm(coeffs.reshape(-1))
    pi = opening_proofs(engine, table, rows, coeffs=coeffs)
    n = k * B

    def per_item(x, name):
        size = bufs.nbytes(x)
        if size == n * 64:
            return bufs.view(x, n, 64)
        if size != k * 64:
            raise ValueError("%s must hold one point per batch (%d) or per item (%d)" % (name, k, n))
        return bufs.expand(bufs.view(x, k, 1, 64), k, B, 64).reshape(n, 64)
    return decrypt_batch_arrays(engine, per_item(D, "D"), pi, per_item(sk, "sk"), C1, C2)


# ----------------------------------------------------------------------------------------------- ragged batches, fused openings
# The same again over batches of any length from 1 to B, as the reference's Digest takes them (afp25_bibe.go:293-305), on
# engine.fr_poly_from_roots_segments and table.openings (include/gpbc_bn254_openings.h): the quotient's coefficients are made in the
# lane that adds their terms, so there is no scratch buffer, no chunk loop and no flag read back.  The rule "the identity occurs
# exactly once in its batch" (afp25_bibe.go:371-381) is decided on the device also for tensors: ok = 0 and an all-zero row, where
# opening_proofs raises.  The functions above keep their behaviour.
def _ragged(engine, table, ids, counts):
    """(flat identity rows, counts): counts=None takes whole batches of B = table.nbase - 1 as _identity_rows does (without its host
    check for duplicates: the device decides); otherwise ids holds sum(counts) identities, integers or scalar rows."""
    B = table.nbase - 1
    if B < 1:
        raise ValueError("the SRS table needs at least two bases (g1 and [tau]_1)")
    if not (bufs.is_torch(ids) or isinstance(ids, np.ndarray) and ids.dtype == np.uint8):
        flat = [int(x) for r in ids for x in (r if isinstance(r, (list, tuple)) else (r,))]
        ids = engine.fr_to_bytes(flat)
    ids = ids.reshape(-1)
    n = bufs.nbytes(ids) // 32
    if bufs.nbytes(ids) != n * 32:
        raise ValueError("ids must hold 32-byte scalars")
    if counts is None:
        if n == 0 or n % B:
            raise ValueError("ids must hold a whole number of batches of B = %d identities" % B)
        counts = [B] * (n // B)
    counts = [int(c) for c in counts]
    if not counts or any(c == 0 for c in counts):
        raise ValueError("identities is empty")
    if any(c < 0 or c > B for c in counts):
        raise ValueError("too many identities for batch size")
    if sum(counts) != n:
        raise ValueError("ids must hold one scalar per identity of every batch (%d)" % sum(counts))
    return ids, counts


def digests_ragged(engine, table, ids, counts):
    """D_j = [f_j(tau)]_1 for batches of counts[j] identities each: [k, 64] (Digest, afp25_bibe.go:293-305, with its two refusals)."""
    ids, counts = _ragged(engine, table, ids, counts)
    return table.msm(engine.fr_poly_from_roots_segments(ids, counts, table.nbase).reshape(-1))


def opening_proofs_fused(engine, table, ids, counts=None):
    """(pi [n, 64], ok [n]): pi[i] = [f_j(tau) / (tau - ids[i])]_1 for every identity i of every batch j, by ONE call of table.openings.
    counts=None: whole batches of B, and then pi is opening_proofs' byte for byte wherever ok = 1.  ok[i] = 0 and an all-zero row where
    the identity does not occur exactly once in its batch; nothing is read back here, so the caller decides when to look at ok."""
    ids, counts = _ragged(engine, table, ids, counts)
    return table.openings(ids, counts)


def decrypt_batches_ragged(engine, table, ids, counts, sk, C1, C2, D=None):
    """(messages [n, 384], ok [n]): decrypt_batches over batches of any length.  ids, counts: as opening_proofs_fused takes them; sk, D:
    [k, 64] (one per batch) or [n, 64] (one per item); C1: [n, 3, 128]; C2: [n, 384].  Rows with ok = 0 come back all zero."""
    ids, counts = _ragged(engine, table, ids, counts)
    n, k = sum(counts), len(counts)
    coeffs = engine.fr_poly_from_roots_segments(ids, counts, table.nbase)
    if D is None:
        D = table.msm(coeffs.reshape(-1))
    pi, ok = table.openings(ids, counts, coeffs=coeffs.reshape(-1))
    of_item = np.repeat(np.arange(k), counts)

    def per_item(x, name):
        if bufs.nbytes(x) not in (k * 64, n * 64):
            raise ValueError("%s must hold one point per batch (%d) or per item (%d)" % (name, k, n))
        x = bufs.view(_plan._placed(x, pi, name), -1, 64)
        return x if x.shape[0] == n else bufs.take(x, of_item)
    m = decrypt_batch_arrays(engine, per_item(D, "D"), pi, per_item(sk, "sk"), C1, C2)
    return bufs.view(m, n, 384) * bufs.view(ok, n, 1), ok
