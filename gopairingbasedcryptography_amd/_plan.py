"""What the scheme planners (bsw07, waters11, lw11, sw05, waters05, gentry06, afp25, and at the end bls01, zss04, bb04sig) share besides the array operations of _buffers:
Python integers as scalar rows, public values put where the batch lives, uniform segment tables, index tables for FixedBase.indexed,
the blinding factor of every Encrypt, a handle that is the caller's or made and closed here, and the items of a batch with ok = 1.
Host-side and engine-agnostic like the planners: an engine is only ever an argument."""
import contextlib

import numpy as np

from . import _buffers as bufs
from ._buffers import R_ORDER

INDEX_NONE = 0xFFFFFFFF          # "no term" in an index row of FixedBase.indexed
NO_ATTRIBUTE = -1                # a padding row's attribute; index_rows turns it into INDEX_NONE


def is_buffer(x):
    return bufs.is_torch(x) or isinstance(x, np.ndarray)


def like_of(*values):
    """the first buffer among the values (its kind is the call's), or an empty host array"""
    return next((x for x in values if is_buffer(x)), np.zeros(0, dtype=np.uint8))


def host(a):
    """a buffer's bytes on the host (a CUDA tensor: the copy waits for its stream)"""
    return a.cpu().numpy() if bufs.is_torch(a) else np.asarray(a)


def scalar_rows(values):
    """Python integers — one, a flat list or generator, or a list of rows — as scalar rows modulo r: a writable [k, 32] uint8 array
    (it may become a tensor).  The values of a batch repeat: each distinct one is converted once."""
    cache = {}

    def row(v):
        b = cache.get(v)
        if b is None:
            b = cache[v] = (int(v) % R_ORDER).to_bytes(32, "little")
        return b
    values = [values] if isinstance(values, (int, np.integer)) else values
    flat = (v for r in values for v in (r if isinstance(r, (list, tuple)) else (r,)))
    return np.frombuffer(b"".join([row(v) for v in flat]), dtype=np.uint8).reshape(-1, 32).copy()


def scalars(v, like, n=None, what=None):
    """A scalar argument of the kind of `like`: a buffer as it is, Python integers through scalar_rows.  With n: checked to hold n
    scalars of that kind, and returned flat."""
    if not is_buffer(v):
        v = bufs.put(scalar_rows(v), like)
    if n is None:
        return v
    if bufs.is_torch(v) != bufs.is_torch(like) or bufs.nbytes(v) != n * 32:
        raise ValueError("%s must hold %d 32-byte scalars of the kind the other arguments are" % (what, n))
    return bufs.flat(bufs.view(v, n * 32))


def _placed(x, like, what):
    """one rule for the kind of a public value: host data is copied and put where `like` is, a tensor is used where it is"""
    if not bufs.is_torch(x):
        return bufs.put(np.array(x, dtype=np.uint8, copy=True).reshape(-1), like)
    if not bufs.is_torch(like):
        raise ValueError("%s must be of the kind the other arguments are" % what)
    return x


def public(x, rows, width, like, what):
    """a public value, [rows, width] of the kind of `like`"""
    if bufs.nbytes(x) != rows * width:
        raise ValueError("%s must hold %d x %d bytes" % (what, rows, width))
    return bufs.view(_placed(x, like, what), rows, width)


def per_item(x, n, rows, width, like, what):
    """[n, rows, width] of the kind of `like` from one value for all n items (expanded, not copied) or one per item"""
    x = _placed(x, like, what)
    if bufs.nbytes(x) not in (rows * width, n * rows * width):
        raise ValueError("%s must hold %d rows of %d bytes, or as many per item" % (what, rows, width))
    x = bufs.view(x, -1, rows, width)
    return x if x.shape[0] == n else bufs.expand(x, n, rows, width)


def segments(n, m):
    """the offset table of n segments of m entries each"""
    return np.arange(0, n * m + 1, m, dtype=np.uint64)


def index_rows(index, like):
    """an index table for FixedBase.indexed of the kind of `like`: uint32 on the host, the same bits as int32 on the device;
    a negative entry (NO_ATTRIBUTE) is INDEX_NONE"""
    idx = np.ascontiguousarray(np.where(index < 0, INDEX_NONE, index).astype(np.uint32))
    return bufs.put(idx.view(np.int32), like) if bufs.is_torch(like) else idx


def blind(engine, base, s, messages, n):
    """base^s_j M_j for the n messages: `base` one GT element of the kind the messages are (gt_exp, gt_mul)"""
    return engine.gt_mul(engine.gt_exp(bufs.flat(bufs.expand(bufs.view(base, 1, 384), n, 384)), bufs.flat(s)), bufs.flat(messages))


@contextlib.contextmanager
def handle(given, make, attr, want, error):
    """The caller's handle (a FixedBase, a ShareTree), or with None one from make() that is closed on the way out.  Either way its
    `attr` must equal `want`: ValueError(error % {"got": ..., "want": ...}) otherwise."""
    h = make() if given is None else given
    try:
        if getattr(h, attr) != want:
            raise ValueError(error % {"got": getattr(h, attr), "want": want})
        yield h
    finally:
        if given is None:
            h.close()


class Good:
    """The items of a batch with ok = 1 (ok: the n flags on the host): only they take part in the group operations, and their
    results go back into n rows whose others stay all zero."""

    def __init__(self, ok, like):
        self.n, self.like, self.index = len(ok), like, np.nonzero(ok)[0]
        self.count = len(self.index)

    def rows(self, a):
        """the good items' rows of a per-item buffer"""
        return bufs.take(a, self.index)

    def scatter(self, msgs, width=384):
        out = bufs.zeros((self.n, width), self.like)
        if self.count:
            out[bufs.put(self.index, self.like)] = bufs.view(msgs, self.count, width)
        return out


# ------------------------------------------------------------------------------------------------ batch verification (bls01, zss04, bb04sig)
P_MODULUS = 21888242871839275222246405745257275088696311157297823662689037894645226208583
# the one of GT as gnark holds it in memory: coefficient C0.B0.A0 = 1 in Montgomery form (2^256 mod p, little-endian), the other eleven zero
GT_ONE = np.frombuffer(((1 << 256) % P_MODULUS).to_bytes(32, "little") + bytes(352), dtype=np.uint8)


def interleave(parts, width):
    """[n * len(parts) * width] flat: row i of every part in turn (the points of a multi-pairing segment per item)"""
    n = bufs.nbytes(parts[0]) // width
    return bufs.flat(bufs.cat([bufs.view(p, n, 1, width) for p in parts], axis=1))


def group_table(n, group):
    """the offset table of n items cut into groups of `group`, the last one short"""
    if not isinstance(group, (int, np.integer)) or isinstance(group, bool) or group < 1:
        raise ValueError("group must be a positive integer")
    return np.append(np.arange(0, n, group, dtype=np.uint64), np.uint64(n))


def weights(rho, like, n):
    """the n weights of a batch verification as scalar rows of the kind of `like`: ONE draw of an rng.Randomness (one stream, weight i
    from index i), or the caller's rows.  Caller-supplied host rows are checked to be non-zero modulo r; rows in a tensor are the
    caller's promise (a zero weight takes its signature out of the equation: a forgery there would pass)."""
    if hasattr(rho, "scalars") and not is_buffer(rho):
        return bufs.flat(bufs.view(rho.scalars(like, n), n * 32))
    rows = scalars(rho, like, n, "rho")
    if not bufs.is_torch(rows):
        r = np.asarray(rows).reshape(n, 32)
        if any(int.from_bytes(x.tobytes(), "little") % R_ORDER == 0 for x in r):
            raise ValueError("the weights rho must be non-zero modulo r")
    return rows


def settle(ok_groups, n, group, like, each):
    """The verdict per item [n] from the verdicts per group: every item of a passing group is accepted; the items of the failing groups
    are gathered — ONE read of the group verdicts — and settled by each(index) -> their verdicts (the per-item Verify)."""
    host = ok_groups.cpu().numpy() if bufs.is_torch(ok_groups) else np.asarray(ok_groups)
    of_item = np.arange(n) // group
    verdict = bufs.copy(bufs.take(bufs.view(ok_groups, -1), of_item))
    bad = np.nonzero(host.reshape(-1)[of_item] == 0)[0]
    if bad.size:
        verdict[bufs.put(bad, like)] = bufs.view(each(bad), -1)
    return verdict
