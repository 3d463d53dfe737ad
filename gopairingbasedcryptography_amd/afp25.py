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

Below the Decrypt forms: KeyGen, Encrypt and ComputeKey (afp25_bibe.go:146-173, 211-269, 327-334) for many identities, labels and
messages at once, whose outputs are the operands of decrypt_batch_arrays / decrypt_batches_ragged.
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


# ----------------------------------------------------------------------------------------------- KeyGen, Encrypt, ComputeKey
# bibe/afp25_bibe/afp25_bibe.go:146-173, 211-269, 327-334 — the rest of the scheme, for many identities, labels and messages at once.  With the
# master key msk, the SRS secret tau, an identity id, a batch label t and randomness r1, r2 in Zr:
#
#     KeyGen       [tau^i]_1, i = 1 .. B     [tau]_2     [msk]_2
#     Encrypt      C1 = ([r1]g2 + [r2][msk]_2,  [r1]([id]_2 - [tau]_2),  [-r2]g2)     C2 = M e(h(t), [msk]_2)^(-r2)
#     ComputeKey   sk = [msk](D + h(t))
#
# Planners only: every stage is an engine entry that exists (fr_mul, g1 / g2_scalar_mul(_base), hash_to_g1, multi_pair_fixed_q, gt_inverse,
# gt_exp, gt_mul, FixedBase.indexed, GTFixedBase.indexed).  Scalars are Python ints, 32-byte rows or tensors; with CUDA tensors nothing but
# the inputs going in and the outputs coming out crosses PCIe.  The master PUBLIC key is a dict of host arrays under the reference struct's
# field names — it is public, B * 64 + 256 bytes, and what srs_table above takes; the public values are put where a batch lives by the
# functions that use them.  Secrets (msk, and tau inside keygen_seeded) stay of the kind they came in.
MAX_B = 1024          # FR_POLY_MAX_B: the longest batch the polynomial kernels behind Digest and Decrypt take
DST_BYTES_G1 = b"Hash Bytes To Element In G1"            # hash_to.DST_BYTES_G1, the tag of hash.BytesToG1 (afp25_bibe_utils.go:10-12)
ROUTES = ("labels", "items")


def _batch_size(B):
    if not isinstance(B, (int, np.integer)) or isinstance(B, bool) or not 1 <= B <= MAX_B:
        raise ValueError("invalid B")                                          # Setup, :114-117, and the polynomial kernels' limit
    return int(B)


def tau_powers(engine, tau, B):
    """[B, 32]: tau^1 .. tau^B modulo r as canonical scalar rows, of the kind of tau (the tauPower chain of KeyGen, :157-162).  By doubling
    where the scalar lives: P[0] = fr_mul(tau, 1), then P[m : 2m] = fr_mul(P[0 : m], P[m - 1]) with the second operand ONE row, broadcast
    (P[m - 1] = tau^m), the last round cut to B — ceil(log2 B) + 1 fr_mul calls in all, and no Python integer when tau is a buffer."""
    B = _batch_size(B)
    tau = _plan.scalars(tau, _plan.like_of(tau), 1, "tau")
    P = bufs.view(engine.fr_mul(tau, bufs.flat(bufs.put(_plan.scalar_rows([1]), tau))), 1, 32)
    while P.shape[0] < B:
        m = P.shape[0]
        more = engine.fr_mul(bufs.flat(P[:min(m, B - m)]), bufs.flat(P[m - 1]))
        P = bufs.cat([P, bufs.view(more, -1, 32)])
    return P


def keygen(engine, B, tau, msk):
    """mpk (KeyGen, :146-173) as a dict of host arrays: G1ExpTauPowers [B, 64] = [tau]_1 .. [tau^B]_1, G2ExpTau [128] = [tau]_2, G2ExpMsk
    [128] = [msk]_2.  The master secret key is the caller's msk.  tau, msk: one scalar each, of one kind.  B < 1 raises
    ValueError("invalid B") as the reference's Setup does (:114-117), and so does B > 1024: the polynomial kernels behind Digest and
    Decrypt take batches of at most 1024, the rule gwww25.keygen has.  Engine calls: tau_powers (fr_mul), ONE g1_scalar_mul_base over the
    B powers, ONE g2_scalar_mul_base over (tau, msk).  The powers of tau are made where tau lives; only the public points come back."""
    B = _batch_size(B)
    like = _plan.like_of(tau, msk)
    tau, msk = _plan.scalars(tau, like, 1, "tau"), _plan.scalars(msk, like, 1, "msk")
    bufs.device_of(tau, msk)
    powers = tau_powers(engine, tau, B)
    in_g1 = engine.g1_scalar_mul_base(bufs.flat(powers))
    in_g2 = bufs.view(engine.g2_scalar_mul_base(bufs.flat(bufs.cat([powers[:1], bufs.view(msk, 1, 32)]))), 2, 128)
    host = lambda x, *shape: np.array(_plan.host(x), dtype=np.uint8, copy=True).reshape(*shape)
    return {"G1ExpTauPowers": host(in_g1, B, 64), "G2ExpTau": host(in_g2[0], 128), "G2ExpMsk": host(in_g2[1], 128)}


def keygen_seeded(engine, B, rng, like=None):
    """(mpk, msk): keygen with the secrets drawn on the device.  ONE draw of two scalars in the reference's order, msk then tau (:147-154)
    — one stream id; the order and the count are part of the interface: they make the key reproducible from the seed.  like: a buffer of
    the kind msk is to be (None: a host array); msk comes back as its 32-byte row.  tau is used and dropped: with a CUDA `like` it is
    drawn, raised to its powers and multiplied into the generators on the device and never becomes a host value.  A refused B draws
    nothing.  The seed is key material: whoever holds it holds the master secret key and the trapdoor."""
    B = _batch_size(B)
    drawn = bufs.view(rng.scalars(np.zeros(0, dtype=np.uint8) if like is None else like, 2), 2, 32)
    return keygen(engine, B, drawn[1], drawn[0]), bufs.copy(bufs.view(drawn[0], 32))          # a copy: msk does not keep the buffer tau sits in alive


def encrypt_tables(engine, mpk):
    """engine.FixedBase(g2=True) over (g2, [msk]_2, [tau]_2): with it every component of C1 is one indexed sum (encrypt_batch, tables=).
    Built once per master public key (6 MiB of device memory); the caller closes it."""
    _, g2 = engine.generators()
    rows = [np.asarray(x, dtype=np.uint8).reshape(1, 128) for x in (g2, mpk["G2ExpMsk"], mpk["G2ExpTau"])]
    return engine.FixedBase(np.concatenate(rows), g2=True)


def label_points(engine, labels, msg_off=None):
    """[L, 64]: h(t) = hash.BytesToG1(t) for every batch label (afp25_bibe_utils.go:10-12) — engine.hash_to_g1 under DST_BYTES_G1.
    labels: a list of byte strings, or the concatenated bytes with msg_off (a device byte buffer with an int64 offset tensor gives a
    tensor), exactly as bn254.hash_to_g1 takes them."""
    return bufs.view(engine.hash_to_g1(labels, DST_BYTES_G1, msg_off), -1, 64)


def label_bases(engine, mpk, points):
    """[L, 384]: b_l = e(h(t_l), [msk]_2)^-1, the reference's b[1] (:227-234), for every label point.  ONE multi_pair_fixed_q over the
    single shared Q = [msk]_2 with one-pair segments (its lines are computed once for all labels), then gt_inverse."""
    if not _plan.is_buffer(points):
        raise ValueError("points must be a uint8 array or a CUDA tensor")
    L = bufs.nbytes(points) // 64
    if bufs.nbytes(points) != L * 64:
        raise ValueError("points are G1 points, rows of 64 bytes")
    if not L:
        return bufs.empty((0, 384), points)
    q = _plan.public(mpk["G2ExpMsk"], 1, 128, points, "G2ExpMsk")
    return bufs.view(engine.gt_inverse(bufs.flat(engine.multi_pair_fixed_q(bufs.flat(points), bufs.flat(q)))), L, 384)


def _pairs_of(a, b, n):
    """[n * 2 * 32] flat: the scalars (a[i], b[i]) of n two-term sums"""
    return bufs.flat(bufs.cat([bufs.view(a, n, 1, 32), bufs.view(b, n, 1, 32)], 1))


def encrypt_batch(engine, mpk, messages, ids, r1, r2, points, label_of=None, bases=None, tables=None, gt_table=None, route="labels"):
    """(C1 [n, 3, 128], C2 [n, 384]) for n messages (GT elements) to n identities with the randomness r1, r2 (Encrypt, :211-269) — the
    operands of decrypt_batch_arrays / decrypt_batches_ragged.  points: label_points' [L, 64]; label_of: a host integer array [n], the
    label of every item as a row of points (None: one label for all, and then L must be 1; an entry outside 0 .. L - 1 is a ValueError
    before any engine call).  ids, r1, r2: n scalars each.  n = 0 gives empty outputs.

    C1 and C2 each by two routes, every combination the same bytes (affine points and GT elements are canonical, and e(P, Q)^k and
    e([k] P, Q) are the same Fp12 element, as bf01.py relies on):

      C1, tables=None   the reference's operations in its order: g2_scalar_mul_base(id) and g2_sub of [tau]_2; g2_scalar_mul of g2 by r1 and
                        of [msk]_2 by r2, g2_add; g2_scalar_mul of [id]_2 - [tau]_2 by r1; g2_scalar_mul of -g2 by r2.  The reference's
                        products with the two infinity entries of A (:218-220) and its power of b[0] = 1 (:258) have fixed bytes — the
                        point at infinity, the one of GT — and are not computed.  With tensors this route also puts four public
                        constants on the device per call — g2, -g2, [tau]_2, [msk]_2, 512 bytes from host arrays (generators, g2_neg,
                        mpk) — besides the inputs; the tables route uploads [msk]_2 for C2 and its index rows, a few bytes.
      C1, tables=       encrypt_tables(engine, mpk): three FixedBase.indexed calls with ONE periodic index row each,
                        C1[0] = indexed([0, 1]; r1, r2), C1[1] = indexed([0, 2]; r1 id, -r1), C1[2] = indexed([0]; -r2), the scalars from
                        fr_mul / fr_neg: no doubling and no variable base.
      C2, "labels"      bases (label_bases' [L, 384]; computed here when None) gathered by label_of, gt_exp by r2, gt_mul with M; or with
                        gt_table — an engine.GTFixedBase over the L bases, built by the caller — gt_table.indexed(label_of; r2, terms=1)
                        and gt_mul: 32 Fp12 products per item and no squaring.  The table costs about 8 ms (for 1 base as for 256) and 4 MiB a
                        base to build: it pays where a label serves thousands of items, not where every batch of B has a label of its own.
      C2, "items"       no pairing per label and no power in GT: P_i = g1_scalar_mul(points[label_of[i]], -r2_i), ONE multi_pair_fixed_q
                        against [msk]_2, gt_mul with M.  For batches whose labels are mostly distinct; bases and gt_table do not apply."""
    if route not in ROUTES:
        raise ValueError('route is "labels" or "items" (got %r)' % (route,))
    if not _plan.is_buffer(messages) or not _plan.is_buffer(points):
        raise ValueError("messages and points must be uint8 arrays or CUDA tensors")
    n, L = bufs.nbytes(messages) // 384, bufs.nbytes(points) // 64
    if bufs.nbytes(messages) != n * 384 or bufs.nbytes(points) != L * 64:
        raise ValueError("messages are GT elements, rows of 384 bytes, and points G1 points, rows of 64")
    if label_of is None:
        if L != 1:
            raise ValueError("label_of=None is one label for all: points must hold one point (got %d)" % L)
    else:
        label_of = np.asarray(label_of)
        if label_of.dtype.kind not in "iu" or label_of.shape != (n,):
            raise ValueError("label_of must be a host integer array of n = %d entries" % n)
        label_of = label_of.astype(np.int64)
        if n and (label_of.min() < 0 or label_of.max() >= L):
            raise ValueError("label_of: every entry must be in 0 .. %d" % (L - 1))
    if route == "items" and (bases is not None or gt_table is not None):
        raise ValueError('bases and gt_table belong to route "labels"')
    if tables is not None and (tables.nbase != 3 or not tables.g2):
        raise ValueError("tables is encrypt_tables(engine, mpk): three G2 bases")
    if gt_table is not None and gt_table.nbase != L:
        raise ValueError("gt_table holds %d bases, the labels need %d" % (gt_table.nbase, L))
    bufs.device_of(messages, points)
    messages, points = bufs.view(messages, n, 384), bufs.view(points, L, 64)
    ids, r1, r2 = (_plan.scalars(x, messages, n, name) for x, name in ((ids, "ids"), (r1, "r1"), (r2, "r2")))
    if bases is not None:
        bases = _plan.public(bases, L, 384, messages, "bases")
    if not n:
        return bufs.empty((0, 3, 128), messages), bufs.empty((0, 384), messages)
    msk2 = bufs.flat(_plan.public(mpk["G2ExpMsk"], 1, 128, messages, "G2ExpMsk"))
    if tables is None:
        g2 = np.asarray(engine.generators()[1], dtype=np.uint8).reshape(128)
        tau2 = bufs.flat(_plan.public(mpk["G2ExpTau"], 1, 128, messages, "G2ExpTau"))
        gen, neg_gen = (bufs.flat(_plan.public(x, 1, 128, messages, "g2")) for x in (g2, engine.g2_neg(g2)))
        a01 = engine.g2_sub(engine.g2_scalar_mul_base(ids), tau2)                                  # [id]_2 - [tau]_2
        c10 = engine.g2_add(engine.g2_scalar_mul(gen, r1), engine.g2_scalar_mul(msk2, r2))
        c11 = engine.g2_scalar_mul(bufs.flat(a01), r1)
        c12 = engine.g2_scalar_mul(neg_gen, r2)
    else:
        row = lambda *index: _plan.index_rows(np.array([index]), messages)
        r1id, nr1, nr2 = engine.fr_mul(r1, ids), engine.fr_neg(r1), engine.fr_neg(r2)
        c10 = tables.indexed(row(0, 1), _pairs_of(r1, r2, n), terms=2)[0]
        c11 = tables.indexed(row(0, 2), _pairs_of(r1id, nr1, n), terms=2)[0]
        c12 = tables.indexed(row(0), bufs.flat(nr2), terms=1)[0]
    C1 = bufs.cat([bufs.view(c, n, 1, 128) for c in (c10, c11, c12)], 1)
    if route == "items":
        mine = bufs.flat(points) if label_of is None else bufs.flat(bufs.take(points, label_of))   # one shared base, or one per scalar
        P = engine.g1_scalar_mul(mine, bufs.flat(engine.fr_neg(r2)))
        blind = engine.multi_pair_fixed_q(bufs.flat(P), msk2)
    elif gt_table is not None:
        index = np.zeros((1, 1), dtype=np.int64) if label_of is None else label_of.reshape(n, 1)        # one periodic row, or a row per item
        blind = gt_table.indexed(_plan.index_rows(index, messages), r2, terms=1)[0]
    else:
        if bases is None:
            bases = label_bases(engine, mpk, points)
        mine = bufs.expand(bufs.view(bases, 1, 384), n, 384) if label_of is None else bufs.take(bufs.view(bases, L, 384), label_of)
        blind = engine.gt_exp(bufs.flat(mine), r2)
    return C1, bufs.view(engine.gt_mul(bufs.flat(blind), bufs.flat(messages)), n, 384)


def encrypt_batch_seeded(engine, mpk, messages, ids, rng, points, label_of=None, bases=None, tables=None, gt_table=None, route="labels"):
    """encrypt_batch with its randomness drawn on the device: TWO draws, r1 [n] then r2 [n], the reference's order (:237-244) — two stream
    ids, none when n == 0 — of the kind the messages are; the order is part of the interface.  The return value is exactly
    encrypt_batch's on the scalars drawn.  The seed is key material: whoever holds it can recompute r2 and with it every message."""
    n = bufs.nbytes(messages) // 384
    r1 = rng.scalars(messages, n)
    return encrypt_batch(engine, mpk, messages, ids, r1, rng.scalars(messages, n), points, label_of=label_of, bases=bases, tables=tables,
                         gt_table=gt_table, route=route)


def compute_key_batch(engine, msk, D, points):
    """sk [k, 64], sk_j = [msk](D_j + h(t_j)) for k (digest, label) pairs (ComputeKey, :327-334): g1_add, then g1_scalar_mul with msk
    expanded to k rows.  D: [k, 64] as digests_ragged gives them; points: label_points' [k, 64], or one point for all; msk: one scalar."""
    if not _plan.is_buffer(D) or not _plan.is_buffer(points):
        raise ValueError("D and points must be uint8 arrays or CUDA tensors")
    k = bufs.nbytes(D) // 64
    if bufs.nbytes(D) != k * 64:
        raise ValueError("D holds G1 points, rows of 64 bytes")
    if bufs.nbytes(points) not in (64, k * 64):
        raise ValueError("points must hold one point per digest (%d), or one for all" % k)
    msk = _plan.scalars(msk, D, 1, "msk")
    points = _plan._placed(points, D, "points")
    if not k:
        return bufs.empty((0, 64), D)
    s = engine.g1_add(bufs.flat(D), bufs.flat(points))
    return bufs.view(engine.g1_scalar_mul(bufs.flat(s), bufs.flat(bufs.expand(bufs.view(msk, 1, 32), k, 32))), k, 64)
