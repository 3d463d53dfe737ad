"""Everything that differs between the two kinds of buffer the package takes: numpy uint8 arrays (host) and torch uint8 tensors
(HBM-resident on the engine's side; the planners also run on CPU tensors over a stand-in engine).  bn254.py normalises its
arguments and gets its outputs here, the scheme planners do their few array operations here; nothing else in the package asks
which kind a buffer is.  Engine-agnostic: this module imports neither the C library nor bn254."""
import numpy as np

R_ORDER = 21888242871839275222246405745257275088548364400416034343698204186575808495617      # the order r of G1, G2 and GT


def is_torch(x):
    return type(x).__module__.startswith("torch")


def device_of(*bufs):
    """The kind of one call's buffers (None entries are skipped): None when all are host data, the tensors' one torch.device when
    all are tensors.  Mixed kinds, or tensors on different devices, are a ValueError."""
    host, tensors = False, []
    for b in bufs:
        if b is None:
            continue
        if isinstance(b, np.ndarray) or not is_torch(b):                      # arrays first: the common case, and the cheaper test
            host = True
        else:
            tensors.append(b)
    if not tensors:
        return None
    if host:
        raise ValueError("the buffers of one call must all be CUDA tensors or all host buffers")
    dev = tensors[0].device
    if any(b.device != dev for b in tensors):
        raise ValueError("the tensors of one call must be on one device (got %s)" % ", ".join(sorted({str(b.device) for b in tensors})))
    return dev


def nbytes(x):
    """number of elements (= bytes, for the uint8 buffers used throughout) of a buffer of either kind"""
    return x.numel() if is_torch(x) else np.asarray(x).size


def rows(x, width, name="buffer"):
    """(flat, n): an input as a flat contiguous uint8 buffer of n whole rows of `width` bytes.  Host data is converted (and copied
    only if it has to be); a tensor is taken as it is, so it must already be contiguous uint8 — its raw address goes to a
    kernel."""
    if not isinstance(x, np.ndarray) and is_torch(x):
        if str(x.dtype) != "torch.uint8" or not x.is_contiguous():
            raise ValueError("%s must be a contiguous uint8 tensor" % name)
        a, size = x.reshape(-1), x.numel()
    else:
        if isinstance(x, (bytes, bytearray)):
            x = np.frombuffer(bytes(x), dtype=np.uint8)
        a = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)
        size = a.size
    if size % width:
        raise ValueError("%s: %d bytes are not a whole number of rows of %d" % (name, size, width))
    return a, size // width


def output(out, shape, dev, name="out"):
    """The output of a call of kind `dev` (device_of): a new uint8 buffer of `shape`, or the caller's `out` after checking that it
    can be written through its raw address — a writable contiguous uint8 array (host), a contiguous uint8 CUDA tensor on `dev`
    (device), of exactly prod(shape) bytes.  A wrong size here would be an out-of-bounds write inside a kernel."""
    if out is None and dev is None:
        return np.empty(shape, dtype=np.uint8)
    n = 1
    for extent in shape:
        n *= extent
    if dev is None:
        if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"] and out.size == n):
            raise ValueError("%s must be a writable contiguous uint8 array of %d bytes" % (name, n))
        return out
    if out is None:
        import torch
        return torch.empty(shape, dtype=torch.uint8, device=dev)
    if device_of(out) is None or rows(out, 1, name)[1] != n:
        raise ValueError("%s must be a contiguous uint8 CUDA tensor of %d bytes" % (name, n))
    if out.device != dev:
        raise ValueError("%s is on %s, expected %s" % (name, out.device, dev))
    return out


def address(x):
    """raw address of a buffer that rows() or output() has passed; anything that is no buffer (a ctypes object) as it is"""
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return x.data_ptr() if is_torch(x) else x


# ------------------------------------------------------------------------------------------------ array operations of the planners
def view(x, *shape):
    """x as uint8 rows of `shape` (host data is converted, a tensor reshaped)"""
    return x.reshape(*shape) if is_torch(x) else np.asarray(x, dtype=np.uint8).reshape(*shape)


def copy(a):
    return a.clone() if is_torch(a) else np.array(a, copy=True)


def flat(a):
    return a.contiguous().reshape(-1) if is_torch(a) else np.ascontiguousarray(a).reshape(-1)


def cat(parts, axis=0):
    if is_torch(parts[0]):
        import torch
        return torch.cat(list(parts), dim=axis)
    return np.concatenate([np.asarray(p) for p in parts], axis=axis)


def expand(a, *shape):
    """broadcast without copying (flat() or cat() make the copy)"""
    return a.expand(*shape) if is_torch(a) else np.broadcast_to(a, shape)


def put(table, like):
    """a host array as a buffer of the kind of `like`, on its device; a tensor already there passes through"""
    if not is_torch(like):
        return table
    if is_torch(table) and table.device == like.device:
        return table
    import torch
    return torch.from_numpy(np.ascontiguousarray(table)).to(like.device)


def take(a, index, axis=0):
    """the entries of `a` along `axis` at the integer array `index`: a host array or, for a tensor, also a tensor on its device"""
    if is_torch(index):
        return a.index_select(axis, index.reshape(-1).long())
    index = np.asarray(index, dtype=np.int64)
    return a.index_select(axis, put(index, a)) if is_torch(a) else np.take(a, index, axis=axis)


def empty(shape, like):
    return output(None, shape, like.device if is_torch(like) else None)


def zeros(shape, like):
    out = empty(shape, like)
    out[...] = 0
    return out


def rows_nonzero(a):
    """per row of a two-dimensional uint8 buffer: 1 where any byte is set, else 0 (uint8 [n], of the buffer's kind)"""
    return (a != 0).any(1).to(a.dtype) if is_torch(a) else (a != 0).any(1).astype(np.uint8)


def unpack_bits(a):
    """[n, W] bytes as [n, 8 W] bits of 0 / 1, the most significant bit of every byte first (numpy.unpackbits' order), uint8 of the
    buffer's kind"""
    if not is_torch(a):
        return np.unpackbits(np.asarray(a, dtype=np.uint8), axis=1)
    shifts = put(np.arange(7, -1, -1, dtype=np.uint8), a)
    return ((a.unsqueeze(-1) >> shifts) & 1).reshape(a.shape[0], -1)


def group_rows(a):
    """(distinct [g, W], inverse [n] int64) of the n >= 1 rows of a two-dimensional uint8 buffer: the distinct rows, in an order of the
    library's choosing, and for every row the position of its value among them — numpy.unique / torch.unique along axis 0 with
    return_inverse, on the rows read as 64-bit words where W allows it (the grouping is the same, a comparison eight times shorter).
    On a CUDA tensor the count g comes back to the host: the call waits for the stream."""
    width = a.shape[1]
    if is_torch(a):
        import torch
        words = a.contiguous().view(torch.int64) if width % 8 == 0 else a
        distinct, inverse = torch.unique(words, dim=0, return_inverse=True)
        return distinct.view(torch.uint8).reshape(-1, width), inverse.reshape(-1)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    distinct, inverse = np.unique(a.view(np.uint64) if width % 8 == 0 else a, axis=0, return_inverse=True)
    return distinct.view(np.uint8).reshape(-1, width), inverse.reshape(-1).astype(np.int64, copy=False)


def range_positions(rows, start, end):
    """[n] int64: for canonical scalar rows [n, 32] the value minus start where it lies in [start, end), else -1, for
    0 <= start <= end < 2^63 — arithmetic on the low 8 bytes once the upper 24 are seen to be zero"""
    if is_torch(rows):
        import torch
        low = rows[:, :8].contiguous().view(torch.int64).reshape(-1)                    # a value of 2^63 or more reads negative: outside
        inside = ~(rows[:, 8:] != 0).any(1) & (low >= start) & (low < end)
        return torch.where(inside, low - start, torch.full_like(low, -1))
    rows = np.asarray(rows, dtype=np.uint8)
    low = np.ascontiguousarray(rows[:, :8]).view("<i8").reshape(-1)
    inside = ~(rows[:, 8:] != 0).any(1) & (low >= start) & (low < end)
    return np.where(inside, low - start, -1).astype(np.int64)


def index_rows_ok(pos, k, a):
    """(index [k, a], ok [k] uint8) of k * a positions with -1 for "none": the positions as FixedBase.indexed takes an index table —
    uint32 on the host, the same bits as int32 on the device, "none" as 0xFFFFFFFF — and ok = 1 where a row holds no "none\""""
    pos = pos.reshape(k, a)
    if is_torch(pos):
        import torch
        return pos.to(torch.int32), (pos >= 0).all(1).to(torch.uint8)
    return np.where(pos < 0, 0xFFFFFFFF, pos).astype(np.uint32), (pos >= 0).all(1).astype(np.uint8)


def rows_equal(a, b):
    """per row of two uint8 buffers of one shape and kind: 1 where the rows hold the same bytes, else 0"""
    return (a == b).all(1).to(a.dtype) if is_torch(a) else (a == b).all(1).astype(np.uint8)
