"""Host-side mirror of the gnark-crypto bn254 surface the reference calls, over the C ABI.

Reference call surface (gnark-crypto v0.19.0 `ecc/bn254`, used e.g. at
signature/bls01_signature/bls_signature.go:45,63,81 and cpabe/bsw07/bsw07_cpabe.go:75,184):

    bn254.Pair(P []G1Affine, Q []G2Affine) (GT, error)            -> pair(P, Q)
    bn254.PairingCheck(P, Q) (bool, error)                        -> pairing_check(P, Q)
    (*G1Affine).ScalarMultiplication(a, s) / ...Base(s)           -> g1_scalar_mul(a, s) / g1_scalar_mul_base(s)
    (*G2Affine).ScalarMultiplication(a, s) / ...Base(s)           -> g2_scalar_mul(a, s) / g2_scalar_mul_base(s)
    (*GT).Exp / Mul / Div / Inverse                               -> gt_exp / gt_mul / gt_div / gt_inverse
    (*G1Affine).Add / Sub / Double, n at a time (and G2)          -> g1_add / g1_sub / g1_double (g2_...)
    bn254.Generators()                                            -> generators()

plus the batched forms the engine adds (pair_batch, multi_pair, pairing_check_batch).  Points and GT
values are numpy uint8 arrays (host) or torch uint8 CUDA tensors (HBM-resident) holding gnark in-memory
structs (Montgomery little-endian limbs): G1 64 B, G2 128 B, GT 384 B; scalars 32-byte little-endian.
Errors follow gnark: length mismatch or empty input to pair/pairing_check raises ValueError("invalid
inputs sizes").  Everything computes on the GPU; a missing extension or device raises EngineError.

Every entry is written once for both kinds of buffer: it normalises its arguments (_buffers.py), checks its own shape
relations, gets its output, and only then touches the engine through _call, which picks the host or the device symbol.
"""
import collections
import ctypes

import numpy as np

from . import _buffers as bufs
from . import _lib
from ._buffers import R_ORDER
from ._lib import EngineError  # noqa: F401  (re-export)

G1_BYTES, G2_BYTES, GT_BYTES, SCALAR_BYTES = 64, 128, 384, 32

# gnark Generators(): g1 = (1, 2), g2 = the standard alt_bn128 twist generator; Montgomery-form bytes.
_G1_GEN_HEX = (
    "9d0d8fc58d435dd33d0bc7f528eb780a2c4679786fa36e662fdf079ac1770a0e3a1b1e8b1b87baa67b168eeb51d6f114"
    "588cf2f0de46ddcc5ebe0f3483ef141c")
_G2_GEN_HEX = (
    "2620bc02d1b5838e72017b493519ebdcdf1a81974726b8fb3b5096af4138571940614ca87d73b4afc4d802585add4360"
    "862fa052fc50e9096b7bea3a83f0fe14f6e96b889dfa9d61789b9ef597d27ffefe7d1b23621a9eff06429eaeeb7efd28"
    "ee5618c7565b0964bb3c7d3222f957dc76103533be35f9558264fd93e6a0a40d")

_slots = None          # HIP ordinal -> slot index of the bound device list (None before init)


def init(device=0):
    """Bind the process to one HIP device (one process per GPU: `init(local_rank)`) or to a list of them (one process
    driving several GPUs: host-pointer batch calls then shard over all of them; CUDA tensors pick their own device)."""
    global _slots
    lib = _lib.load()
    devs = [int(device)] if isinstance(device, int) else [int(d) for d in device]
    arr = (ctypes.c_int * len(devs))(*devs)
    _lib.check(lib.gpbc_init_devices(arr, len(devs)))
    _slots = {}
    for i, d in enumerate(devs):
        _slots.setdefault(d, i)
    return device


def init_all():
    """Bind every visible device; returns their number."""
    n = _lib.check(_lib.load().gpbc_device_count())
    init(list(range(n)))
    return n


def num_devices():
    return int(_lib.load().gpbc_num_devices())


def release_workspaces():
    """Hand the library's grow-only device buffers (workspaces, per-call scratch) back to the driver; they regrow on demand."""
    _ensure_init()
    _lib.check(_lib.load().gpbc_release_workspaces())


def small_call_stats():
    """(batches, calls, largest_batch, failed_in_shared_batches) of the small-call combiner since the library was loaded
    (gpbc_small_call_stats); needs no device."""
    v = [ctypes.c_uint64() for _ in range(4)]
    _lib.check(_lib.load().gpbc_small_call_stats(*(ctypes.byref(x) for x in v)))
    return tuple(int(x.value) for x in v)


def shutdown():
    global _slots
    for t in list(_gen_tables.values()):
        t.close()
    _gen_tables.clear()
    _lib.check(_lib.load().gpbc_shutdown())
    _slots = None


def _ensure_init():
    if _slots is None:
        init(0)


# --------------------------------------------------------------------------------------- the one way into the library
def _current_stream():
    import torch
    return torch.cuda.current_stream()


def _torch_stream():
    return _current_stream().cuda_stream


def _bind(dev):
    """Make the tensors' device the calling thread's current one; it must be a GPU, and one of the bound devices."""
    if dev.type != "cuda":
        raise ValueError("device buffers must be CUDA tensors (host data goes in as numpy arrays)")
    _ensure_init()
    idx = dev.index if dev.index is not None else 0
    if idx not in _slots:
        raise ValueError("device %s is not bound: call bn254.init() with it" % dev)
    _lib.check(_lib.load().gpbc_set_device(_slots[idx]))


def _call(name, dev, *args):
    """One checked C call on arguments that are already validated: gpbc_<name> for host buffers (dev is None), gpbc_<name>_dev for
    tensors on `dev` (bufs.device_of), bound first and given the current torch stream as the last argument — enqueued, not
    synchronised.  Arrays and tensors among `args` go as their raw addresses, everything else as it is; the declared argtypes
    (_lib.SIGNATURES) do the conversion."""
    args = [a if a is None or a.__class__ is int else bufs.address(a) for a in args]
    if dev is None:
        _ensure_init()
        return _lib.check(getattr(_lib.load(), "gpbc_" + name)(*args))
    _bind(dev)
    return _lib.check(getattr(_lib.load(), "gpbc_%s_dev" % name)(*args, _torch_stream()))


def _workspace(workspace, need, dev):
    """(buffer, bytes) for the device forms that take a caller-side workspace of at least `need` bytes: the caller's, or a new one"""
    if workspace is None:
        workspace = bufs.output(None, (max(need, 1),), dev)
    elif bufs.device_of(workspace) != dev:
        raise ValueError("workspace must be a CUDA tensor on %s" % dev)
    workspace, size = bufs.rows(workspace, 1, "workspace")
    if size < need:
        raise ValueError("workspace holds %d bytes, needs %d" % (size, need))
    return workspace, size


def _device_segments(seg_off, dev, what):
    """number of segments of a segment table in device memory: it is read as k + 1 uint64 by the kernel, so its dtype is checked here"""
    if str(seg_off.dtype) not in ("torch.int64", "torch.uint64") or not seg_off.is_cuda or not seg_off.is_contiguous() or seg_off.device != dev:
        raise ValueError("a device segment table must be a contiguous int64 / uint64 CUDA tensor on the %s' device" % what)
    if seg_off.numel() < 2:
        raise ValueError("invalid inputs sizes")
    return seg_off.numel() - 1


def _check_segments(dev, seg_off, n, k):
    """a device segment table must start at 0, be monotone and end at n: checked on the device before a kernel walks it"""
    try:
        _call("check_segments", dev, seg_off, n, k)
    except EngineError as e:
        raise ValueError("invalid inputs sizes: %s" % e) from None


def scalars_to_bytes(scalars):
    """ints (any sign/size; reduced mod r like fr.Element.BigInt round trips) or a uint8 buffer -> n x 32 LE bytes."""
    if isinstance(scalars, (bytes, bytearray, np.ndarray)) or bufs.is_torch(scalars):
        return scalars
    if isinstance(scalars, int):
        scalars = [scalars]
    return np.frombuffer(b"".join((int(s) % R_ORDER).to_bytes(32, "little") for s in scalars), dtype=np.uint8)


def generators():
    """(g1, g2) affine generators as uint8 arrays (gnark: `_, _, g1, g2 := bn254.Generators()`)."""
    return (np.frombuffer(bytes.fromhex(_G1_GEN_HEX), dtype=np.uint8).copy(),
            np.frombuffer(bytes.fromhex(_G2_GEN_HEX), dtype=np.uint8).copy())


P_MODULUS = 21888242871839275222246405745257275088696311157297823662689037894645226208583


def _fp_neg_bytes(b):
    """p - y on one 32-byte little-endian Montgomery value (the negation of yR mod p is (p - y)R mod p); 0 stays 0."""
    v = int.from_bytes(bytes(b), "little")
    return ((P_MODULUS - v) % P_MODULUS).to_bytes(32, "little")


def g1_neg(pt):
    """G1Affine.Neg on one 64-byte point (host side, like the field negation of include/gpbc_bn254.hpp): (x, -y)."""
    b = np.asarray(pt, dtype=np.uint8).reshape(G1_BYTES).tobytes()
    return np.frombuffer(b[:32] + _fp_neg_bytes(b[32:]), dtype=np.uint8).copy()


def g2_neg(pt):
    """G2Affine.Neg on one 128-byte point: (x, -y) with y in Fp2."""
    b = np.asarray(pt, dtype=np.uint8).reshape(G2_BYTES).tobytes()
    return np.frombuffer(b[:64] + _fp_neg_bytes(b[64:96]) + _fp_neg_bytes(b[96:]), dtype=np.uint8).copy()


def _rowwise(name, out_width, *operands, out=None):
    """out[i] = f(operand_0[i], operand_1[i], ...): the entries of the form gpbc_<name>(operands..., n, out).  Each operand is
    (buffer, row width, argument name); all hold n rows."""
    dev = bufs.device_of(*(x for x, _, _ in operands))
    flat = [bufs.rows(x, width, what) for x, width, what in operands]
    n = flat[0][1]
    if any(m != n for _, m in flat):
        raise ValueError("operand sizes differ: %s" % ", ".join("%s holds %d rows" % (o[2], m) for o, (_, m) in zip(operands, flat)))
    out = bufs.output(out, (n, out_width), dev)
    _call(name, dev, *(x for x, _ in flat), n, out)
    return out


def _binary(name, width, a, b, out):
    """out[i] = a[i] OP b[j] (b is None: a unary entry); j = i for one b per a, j = 0 for a single b.  `out` may be `a`, or `b` when
    it holds one row per element (gnark's p.Add(p, q)).  An empty batch returns an empty result without touching the engine."""
    dev = bufs.device_of(a, b)
    a, n = bufs.rows(a, width, "a")
    operands = [a]
    if b is not None:
        b, nb = bufs.rows(b, width, "b")
        if nb not in (1, n):
            raise ValueError("need one b or one b per a (got %d for %d)" % (nb, n))
        operands += [b, nb]
    out = bufs.output(out, (n, width), dev)
    if n:
        _call(name + "_batch", dev, *operands, n, out)
    return out


# --------------------------------------------------------------------------------------- pairings
def _pairs(P, Q, host_only=False):
    """(dev, P, n, Q, nq) of the pairing entries.  Points of different kinds are refused with gnark's text, as a length mismatch is;
    the host-only entries refuse tensors, whose addresses must never reach a host-pointer symbol."""
    if bufs.is_torch(P) != bufs.is_torch(Q):
        raise ValueError("invalid inputs sizes")
    dev = bufs.device_of(P, Q)
    if host_only and dev is not None:
        raise ValueError("this entry takes host buffers only (numpy arrays), not tensors")
    (P, n), (Q, nq) = bufs.rows(P, G1_BYTES, "P"), bufs.rows(Q, G2_BYTES, "Q")
    return dev, P, n, Q, nq


def pair_batch(P, Q, out=None):
    """n independent pairings: out[i] = Pair([P[i]], [Q[i]])."""
    dev, P, n, Q, nq = _pairs(P, Q)
    if nq != n or n == 0:
        raise ValueError("invalid inputs sizes")
    out = bufs.output(out, (n, GT_BYTES), dev)
    _call("pair_batch", dev, P, Q, n, out)
    return out


def multi_pair(P, Q, seg_off, out=None, workspace=None):
    """k products of pairings: out[j] = Pair(P[seg_off[j]:seg_off[j+1]], Q[...]) with one final exponentiation each."""
    dev, P, n, Q, nq = _pairs(P, Q)
    if nq != n:
        raise ValueError("invalid inputs sizes")
    if bufs.is_torch(seg_off):
        bufs.device_of(P, seg_off)                                           # a device table goes with device points only
        # The third form, and the reason this body names the buffer kind: a segment table that already lives in device memory.  It
        # is validated by a kernel, and gpbc_multi_pair_dev takes n and a caller-side workspace, which the other two forms do not.
        k = _device_segments(seg_off, dev, "points")
        out = bufs.output(out, (k, GT_BYTES), dev)
        _check_segments(dev, seg_off, n, k)
        ws = _workspace(workspace, _lib.load().gpbc_multi_pair_workspace_bytes(n, k), dev)
        _call("multi_pair", dev, P, Q, seg_off, n, k, out, *ws)
        return out
    # segment table on the host, for host points and for device points (there the engine can cut segments into chunks that share
    # their Miller squarings): the two symbols take the same arguments
    seg = np.ascontiguousarray(seg_off, dtype=np.uint64)
    k = seg.size - 1
    if k < 1 or int(seg[-1]) != n:
        raise ValueError("invalid inputs sizes")
    out = bufs.output(out, (k, GT_BYTES), dev)
    _call("multi_pair" if dev is None else "multi_pair_hostseg", dev, P, Q, seg, k, out)
    return out


def multi_pair_fixed_q(P, Q):
    """k products over ONE shared list of m G2 points: out[j] = Pair(P[j*m:(j+1)*m], Q).  The lines of every Q_i are computed
    once for all k segments (a decryption key against k ciphertexts; gnark: PrecomputeLines / MillerLoopFixedQ)."""
    dev, P, n, Q, m = _pairs(P, Q)
    if m < 1 or n < m or n % m:
        raise ValueError("invalid inputs sizes")
    out = bufs.output(None, (n // m, GT_BYTES), dev)
    _call("multi_pair_fixed_q", dev, P, Q, m, n // m, out)
    return out


def _host_pairs(P, Q, seg_off):
    """(P, Q, seg, k) of the host-only entries (pair, pairing_check, pairing_check_batch), refused like gnark's"""
    _, P, n, Q, nq = _pairs(P, Q, host_only=True)
    seg = np.ascontiguousarray([0, n] if seg_off is None else seg_off, dtype=np.uint64)
    k = seg.size - 1
    if n == 0 and seg_off is None or nq != n or k < 1 or int(seg[-1]) != n:
        raise ValueError("invalid inputs sizes")
    return P, Q, seg, k


def pair(P, Q):
    """bn254.Pair(P, Q): the product of the pairings of all (P[i], Q[i]); one 384-byte GT."""
    P, Q, seg, _ = _host_pairs(P, Q, None)
    return multi_pair(P, Q, seg)[0]


def _pairing_checks(P, Q, seg, k):
    ok = np.empty(k, dtype=np.uint8)
    _call("pairing_check", None, P, Q, seg, k, ok)
    return ok.astype(bool)


def pairing_check_batch(P, Q, seg_off):
    return _pairing_checks(*_host_pairs(P, Q, seg_off))


def pairing_check(P, Q):
    """bn254.PairingCheck(P, Q): product of pairings == 1."""
    return bool(_pairing_checks(*_host_pairs(P, Q, None))[0])


def miller_loop(P, Q):
    return _rowwise("miller_loop", GT_BYTES, (P, G1_BYTES, "P"), (Q, G2_BYTES, "Q"))


def final_exp(F):
    return _rowwise("final_exp", GT_BYTES, (F, GT_BYTES, "F"))


# --------------------------------------------------------------------------------------- scalar multiplication
def _scalar_mul(group, width, bases, scalars, out):
    scalars = scalars_to_bytes(scalars)
    dev = bufs.device_of(bases, scalars)
    (bases, nbase), (scalars, n) = bufs.rows(bases, width, "bases"), bufs.rows(scalars, SCALAR_BYTES, "scalars")
    if nbase not in (1, n) and (nbase < 1 or nbase > n or n % nbase):
        raise ValueError("need one base, one base per scalar, or one base per row of n / nbase scalars (got %d bases for %d scalars)" % (nbase, n))
    out = bufs.output(out, (n, width), dev)
    _call(group + "_scalar_mul_batch", dev, bases, nbase, scalars, n, out)
    return out


# The row form of g1 / g2_scalar_mul as csrc/rows29.hip.hpp lays it out (tests and tools/scalar_mul_rows_bench.py derive their shapes
# from these; tests/test_scalar_mul_rows.py holds them against the header): G1 rows of ROWS_TABLE_MIN .. ROWS_TABLE_MAX - 1 scalars get
# a window table of ROWS_TABLE_BYTES per base, built for a pass of at most rows_pass_bases(nbase, m) bases at a time; the window bases
# the tables grow from are made for up to ROWS_GROUP_BASES bases ahead of their passes.
ROWS_TABLE_MIN, ROWS_TABLE_MAX, ROWS_TABLE_BYTES, ROWS_PASS_OUTPUTS, ROWS_TABLE_CAP, ROWS_GROUP_BASES = 32, 16384, 61440, 1 << 18, 1 << 30, 1 << 16


def rows_pass_bases(nbase, m):
    """bases per pass of the G1 row tables for nbase bases of m scalars each (csrc/rows29.hip.hpp: rows_pass_bases)"""
    return min(nbase, max(1, min(ROWS_PASS_OUTPUTS // m, ROWS_TABLE_CAP // ROWS_TABLE_BYTES)))


# The G2 row tables as csrc/rows29_g2.hip.hpp lays them out (tests/test_scalar_mul_rows_g2.py holds these against the header): G2 rows of
# ROWS_G2_TABLE_MIN .. ROWS_TABLE_MAX - 1 scalars get a window table of ROWS_G2_TABLE_BYTES per base over the four GLS quarters (17 windows
# of 15 rows of 256 bytes), built for a pass of at most rows_g2_pass_bases(nbase, m) bases at a time from window bases made for up to
# ROWS_G2_GROUP_BASES bases ahead of their passes.  ROWS_G2_TABLE_MIN is measured (profiles/shared_base_rows_g2.json).
ROWS_G2_TABLE_MIN, ROWS_G2_TABLE_BYTES, ROWS_G2_PASS_OUTPUTS, ROWS_G2_TABLE_CAP, ROWS_G2_GROUP_BASES = 16, 65280, 1 << 18, 1 << 30, 1 << 16


def rows_g2_pass_bases(nbase, m):
    """bases per pass of the G2 row tables for nbase bases of m scalars each (csrc/rows29_g2.hip.hpp: rows_g2_pass_bases)"""
    return min(nbase, max(1, min(ROWS_G2_PASS_OUTPUTS // m, ROWS_G2_TABLE_CAP // ROWS_G2_TABLE_BYTES)))


def g1_scalar_mul(bases, scalars, out=None):
    """out[i] = new(G1Affine).ScalarMultiplication(&bases[i], scalars[i]): one base per scalar, ONE shared base, or — the row form —
    nbase bases for n = nbase * m scalars, row-major: out[j * m + i] = [scalars[j * m + i]] bases[j], a base with its own row of m
    scalars (the authority secrets against one user's H(GID)).  The bytes are those of the call on the bases repeated m times.  Any
    other count of bases is a ValueError.  numpy arrays in, numpy array out; CUDA tensors in, CUDA tensor out, enqueued on the
    current torch stream."""
    return _scalar_mul("g1", G1_BYTES, bases, scalars, out)


def g2_scalar_mul(bases, scalars, out=None):
    """g1_scalar_mul in G2, the row form (out[j * m + i] = [scalars[j * m + i]] bases[j]) included."""
    return _scalar_mul("g2", G2_BYTES, bases, scalars, out)


# What differs between the segmented reductions (gt_multi_exp, g1 / g2_multi_scalar_mul) for _segmented_reduce: the C entry, the element
# width, the words of the messages, the workspace-size call (lib, n, n_seg) and the alignment the kernels need of the workspace.
_SegRed = collections.namedtuple("_SegRed", "entry width x_name k_name elements per_element shared int_range ws_bytes ws_align")


def _segmented_reduce(op, x, k, seg_off, out, workspace):
    """out[s] = the reduction of x[seg_off[s]:seg_off[s+1]] with one k per element, one list of k for segments of equal length, or none"""
    if isinstance(k, int):
        k = [k]
    if isinstance(k, (list, tuple)):
        if any(not 0 <= int(e) < (1 << 256) for e in k):
            raise ValueError(op.int_range)
        k = np.frombuffer(b"".join(int(e).to_bytes(32, "little") for e in k), dtype=np.uint8)
    dev_table = bufs.is_torch(seg_off)
    dev = bufs.device_of(x, seg_off if dev_table else None, k if bufs.is_torch(k) else None)     # a host k may go with device bases
    x, n = bufs.rows(x, op.width, op.x_name)
    if dev_table:
        n_seg = _device_segments(seg_off, dev, op.elements)
    else:
        seg = np.ascontiguousarray(seg_off, dtype=np.uint64).reshape(-1)
        n_seg = seg.size - 1
        if n_seg < 1 or int(seg[0]) != 0 or int(seg[-1]) != n or (np.diff(seg.astype(np.int64)) < 0).any():
            raise ValueError("seg_off must have n_seg + 1 >= 2 non-decreasing entries from 0 to the number of %s" % op.elements)
    nk = 0
    if k is not None:
        k, nk = bufs.rows(k, SCALAR_BYTES, op.k_name)
        if nk != n:
            if nk > n or nk * n_seg != n:
                raise ValueError("%s must hold %s, or one list for segments of equal length (nk = %d, n = %d, n_seg = %d)" % (op.k_name, op.per_element, nk, n, n_seg))
            if not dev_table and (np.diff(seg.astype(np.int64)) != nk).any():
                raise ValueError("a shared %s list of %d needs segments of exactly %d %s" % (op.shared, nk, nk, op.elements))
    out = bufs.output(out, (n_seg, op.width), dev)
    if dev is None:
        _call(op.entry, None, x, k, nk, seg, n_seg, out)
        return out
    # The device form is a call of its own, which is why this body names the buffer kind: the *_dev entry walks a segment table in
    # device memory (the caller's, validated by a kernel, or the host table copied there), takes n and a caller-side workspace, and
    # accepts a host list of k next to device bases.
    if k is not None and not bufs.is_torch(k):
        k = bufs.put(k.copy(), x)
    if dev_table:
        _check_segments(dev, seg_off, n, n_seg)
        import torch
        if nk != n and k is not None and bool((seg_off.view(torch.int64).diff() != nk).any()):
            raise ValueError("a shared %s list of %d needs segments of exactly %d %s" % (op.shared, nk, nk, op.elements))
    else:
        seg_off = bufs.put(seg.astype(np.int64), x)
    ws = _workspace(workspace, op.ws_bytes(_lib.load(), n, n_seg), dev)
    if bufs.address(ws[0]) % op.ws_align:
        raise ValueError("workspace must be %d-byte aligned" % op.ws_align)
    _call(op.entry, dev, x, k, nk, seg_off, n, n_seg, out, *ws)
    return out


def _multi_scalar_mul(group, width, bases, scalars, seg_off, out, workspace):
    """out[s] = sum_{i in [seg_off[s], seg_off[s+1])} [scalars[i]] bases[i] (include/gpbc_bn254_ext.h): gt_multi_exp's shape in G1 / G2"""
    op = _SegRed(group + "_multi_scalar_mul", width, "bases", "scalars", "points", "one per point", "scalar",
                 "scalars must be in [0, 2^256) (they act as their residue mod r)",
                 lambda lib, n, n_seg: lib.gpbc_multi_scalar_mul_workspace_bytes(n, n_seg, int(group == "g2")), 16)
    if scalars is not None and not isinstance(scalars, (int, list, tuple)):
        scalars = scalars_to_bytes(scalars)                                  # a buffer as it is; any other iterable of integers mod r
    return _segmented_reduce(op, bases, scalars, seg_off, out, workspace)


def g1_multi_scalar_mul(bases, scalars, seg_off, out=None, workspace=None):
    """out[s] = sum_{i in [seg_off[s], seg_off[s+1])} [scalars[i]] bases[i] in G1: the per-item sums of a few scalar multiples of
    ciphertext points (S = sum_x [-w_x] C_x of Waters11 Decrypt) as one call, every term with ScalarMultiplication's semantics, the
    doublings shared by four terms, one affine conversion per segment.  scalars: one per point, or ONE list of m when every segment
    has exactly m points (the weights of a policy against many ciphertexts), or None for the plain sums; Python ints must be in
    [0, 2^256).  numpy arrays in, numpy array out; CUDA tensors in (seg_off a host sequence, or an int64 / uint64 CUDA tensor that
    is then validated on the device), CUDA tensor out, enqueued on the current torch stream.  Arguments are checked before the
    engine is touched."""
    return _multi_scalar_mul("g1", G1_BYTES, bases, scalars, seg_off, out, workspace)


def g2_multi_scalar_mul(bases, scalars, seg_off, out=None, workspace=None):
    """g1_multi_scalar_mul in G2 (sum_x w_x c3x of LW11 Decrypt)."""
    return _multi_scalar_mul("g2", G2_BYTES, bases, scalars, seg_off, out, workspace)


def g1_sum_segments(pts, seg_off):
    """out[s] = sum pts[seg_off[s]:seg_off[s+1]]: g1_multi_scalar_mul without scalars (no tables, no doublings)."""
    return g1_multi_scalar_mul(pts, None, seg_off)


def g2_sum_segments(pts, seg_off):
    return g2_multi_scalar_mul(pts, None, seg_off)


# --------------------------------------------------------------------------------------- elementwise group law
def g1_add(a, b, out=None):
    """out[i] = a[i] + b[i] (or + b[0] for a single b): G1Affine.Add, batched.  A single Add is cheaper in gnark on the host."""
    return _binary("g1_add", G1_BYTES, a, b, out)


def g1_sub(a, b, out=None):
    """out[i] = a[i] - b[i] (or - b[0]): G1Affine.Sub, batched."""
    return _binary("g1_sub", G1_BYTES, a, b, out)


def g1_double(a, out=None):
    """out[i] = 2 a[i]: G1Affine.Double, batched."""
    return _binary("g1_double", G1_BYTES, a, None, out)


def g2_add(a, b, out=None):
    """out[i] = a[i] + b[i] (or + b[0]): G2Affine.Add, batched (e.g. [H(m_i)]g2 + pk)."""
    return _binary("g2_add", G2_BYTES, a, b, out)


def g2_sub(a, b, out=None):
    return _binary("g2_sub", G2_BYTES, a, b, out)


def g2_double(a, out=None):
    return _binary("g2_double", G2_BYTES, a, None, out)


# --------------------------------------------------------------------------------------- scalar field Fr
# fr.Element arithmetic on the scalar format (32-byte little-endian plain integers): inputs are any value < 2^256 and act as their
# residue mod r, outputs are canonical — ready to be the `scalars` of g1_scalar_mul, FixedBase.msm and gt_exp without leaving HBM.
FR_POLY_MAX_B = 1024


def fr_to_bytes(values):
    """ints in [0, 2^256) (NOT reduced: the device does that) or a uint8 buffer -> the scalar rows as a flat uint8 array."""
    if isinstance(values, np.ndarray):
        if values.dtype != np.uint8:
            raise ValueError("scalar buffers must be uint8 (got %s)" % values.dtype)
        a = np.ascontiguousarray(values).reshape(-1)
    elif isinstance(values, (bytes, bytearray)):
        a = np.frombuffer(bytes(values), dtype=np.uint8)
    else:
        if isinstance(values, int):
            values = [values]
        vals = [int(v) for v in values]
        if any(v < 0 or v >> 256 for v in vals):
            raise ValueError("scalars must lie in [0, 2^256)")
        a = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint8)
    if a.size % SCALAR_BYTES:
        raise ValueError("buffer length %d is not a multiple of %d" % (a.size, SCALAR_BYTES))
    return a


def fr_to_ints(rows):
    """scalar rows (numpy, or a CUDA tensor: copied to the host) -> Python ints"""
    if bufs.is_torch(rows):
        rows = rows.cpu().numpy()
    b = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, SCALAR_BYTES)
    return [int.from_bytes(r.tobytes(), "little") for r in b]


def _fr_in(v):
    """a scalar argument: a tensor as it is, host values through fr_to_bytes (None stays None)"""
    return v if v is None or bufs.is_torch(v) else fr_to_bytes(v)


def fr_add(a, b, out=None):
    """out[i] = a[i] + b[i] mod r (or + b[0] for a single b): fr.Element.Add, batched."""
    return _binary("fr_add", SCALAR_BYTES, _fr_in(a), _fr_in(b), out)


def fr_sub(a, b, out=None):
    return _binary("fr_sub", SCALAR_BYTES, _fr_in(a), _fr_in(b), out)


def fr_mul(a, b, out=None):
    return _binary("fr_mul", SCALAR_BYTES, _fr_in(a), _fr_in(b), out)


def fr_neg(a, out=None):
    return _binary("fr_neg", SCALAR_BYTES, _fr_in(a), None, out)


def fr_inverse(a, out=None):
    """fr.Element.Inverse, batched: 1 / a[i] mod r, and 0 where a[i] is 0 mod r."""
    return _binary("fr_inverse", SCALAR_BYTES, _fr_in(a), None, out)


def fr_from_mont(a, out=None):
    """fr.Element in-memory words (4 x uint64, x 2^256 mod r) -> the scalar format."""
    return _binary("fr_from_mont", SCALAR_BYTES, _fr_in(a), None, out)


def fr_to_mont(a, out=None):
    """the scalar format -> canonical fr.Element in-memory words."""
    return _binary("fr_to_mont", SCALAR_BYTES, _fr_in(a), None, out)


def fr_dot_segments(a, b, seg_off, out=None, workspace=None):
    """out[s] = sum_{i in [seg_off[s], seg_off[s+1])} a[i] b[i] mod r (include/gpbc_bn254_verify.h): gt_multi_exp's shape in Fr, with
    sums for products.  b: one scalar per element, or ONE list of m when every segment has exactly m elements, or None for the plain
    sum of a.  Scalar rows (any value below 2^256, acting as its residue) or Python ints in [0, 2^256); the sums are canonical.  numpy
    arrays in, numpy array out; CUDA tensors in (seg_off a host sequence, or an int64 / uint64 CUDA tensor that is then validated on
    the device), CUDA tensor out, enqueued on the current torch stream.  Arguments are checked before the engine is touched."""
    op = _SegRed("fr_dot_segments", SCALAR_BYTES, "a", "b", "elements", "one second operand per element", "second operand",
                 "scalars must be in [0, 2^256) (they act as their residue mod r)", lambda lib, n, n_seg: lib.gpbc_fr_dot_segments_workspace_bytes(n, n_seg), 16)
    return _segmented_reduce(op, _fr_in(a), b, seg_off, out, workspace)


def fr_sum_segments(a, seg_off):
    """out[s] = sum a[seg_off[s]:seg_off[s+1]] mod r: fr_dot_segments without a second operand."""
    return fr_dot_segments(a, None, seg_off)


def _fr_rows_arg(v, per_row, what):
    """(flat buffer, rows, per_row) of a polynomial / set / node argument: nested Python ints [rows][per_row] (per_row may then be
    None), or scalar rows as a uint8 array / bytes / CUDA tensor together with per_row"""
    if not bufs.is_torch(v) and not isinstance(v, (np.ndarray, bytes, bytearray)):
        rows = [list(r) for r in v]
        per_row = len(rows[0]) if rows and per_row is None else per_row
        if any(len(r) != per_row for r in rows):
            raise ValueError("%s: every row needs %s scalars" % (what, per_row))
        v = [s for r in rows for s in r]
    if not isinstance(per_row, (int, np.integer)) or isinstance(per_row, bool) or not 1 <= int(per_row) <= FR_POLY_MAX_B:
        raise ValueError("%s: the row length must be in 1 .. %d (got %s)" % (what, FR_POLY_MAX_B, per_row))
    per_row = int(per_row)
    flat, nscalars = bufs.rows(_fr_in(v), SCALAR_BYTES, what)
    if nscalars % per_row:
        raise ValueError("%s: %d scalars are not a whole number of rows of %d" % (what, nscalars, per_row))
    return flat, nscalars // per_row, per_row


def fr_poly_from_roots(roots, B=None, out=None):
    """k polynomials prod_{i<B} (X - roots[j][i]), coefficients constant term first: [k, B + 1, 32] (computePolynomialCoeffs).
    roots: [k][B] Python ints, or k x B scalar rows as a uint8 array / CUDA tensor together with B."""
    dev = bufs.device_of(roots) if bufs.is_torch(roots) else None
    r, k, B = _fr_rows_arg(roots, B, "roots")
    out = bufs.output(out, (k, B + 1, SCALAR_BYTES), dev)
    if k:
        _call("fr_poly_from_roots", dev, r, B, k, out)
    return out


def _segment_counts(counts, n, longest, what):
    """(seg_off [k + 1] uint64 on the host, k) of n elements cut into segments: counts a list of segment lengths that sum to n, or an
    int B for whole batches of B.  No segment may be longer than `longest`."""
    if isinstance(counts, (int, np.integer)) and not isinstance(counts, bool):
        B = int(counts)
        if B < 1 or n % B:
            raise ValueError("%s: %d elements are not a whole number of batches of %s" % (what, n, counts))
        lens = np.full(n // B, B, dtype=np.int64)
    else:
        try:
            lens = np.array([int(c) for c in counts], dtype=np.int64).reshape(-1)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("%s: counts is a list of segment lengths or one batch size" % what) from None
    if lens.size >= 1 << 31:
        raise ValueError("%s: too many segments for one call (%d)" % (what, lens.size))
    if lens.size and (int(lens.min()) < 0 or int(lens.max()) > longest):
        raise ValueError("%s: a segment holds between 0 and %d elements (got %d .. %d)" % (what, longest, int(lens.min()), int(lens.max())))
    if int(lens.sum()) != n:
        raise ValueError("%s: the segments hold %d elements, the buffer %d" % (what, int(lens.sum()), n))
    seg = np.zeros(lens.size + 1, dtype=np.uint64)
    np.cumsum(lens, out=seg[1:])
    return seg, lens.size


def _flat_scalars(v, what):
    """(flat buffer, n) of a list of scalars: Python ints (flat, or a list of rows of any lengths), scalar rows as a uint8 array / bytes /
    CUDA tensor"""
    if not bufs.is_torch(v) and not isinstance(v, (np.ndarray, bytes, bytearray)):
        v = [v] if isinstance(v, (int, np.integer)) else list(v)
        v = [s for r in v for s in (r if isinstance(r, (list, tuple)) else (r,))]
    return bufs.rows(_fr_in(v), SCALAR_BYTES, what)


def fr_poly_from_roots_segments(roots, counts, stride, out=None):
    """k polynomials prod_{i in segment j} (X - roots[i]) over segments of any length up to 1024 (include/gpbc_bn254_openings.h): row j of
    the result [k, stride, 32] holds the m_j + 1 coefficients, constant term first, then zeros; an empty segment gives the polynomial 1.
    roots: n Python ints, or n scalar rows as a uint8 array / CUDA tensor; counts: the k segment lengths, or an int B for whole batches of
    B; stride: scalars per row, at least the longest segment + 1.  On full batches with stride = B + 1 the bytes are fr_poly_from_roots'."""
    r, n = _flat_scalars(roots, "roots")
    dev = bufs.device_of(r, out)
    if not isinstance(stride, (int, np.integer)) or isinstance(stride, bool) or not 1 <= int(stride) <= 1 << 24:
        raise ValueError("stride must be in 1 .. 2^24 (got %s)" % (stride,))
    stride = int(stride)
    seg, k = _segment_counts(counts, n, min(FR_POLY_MAX_B, stride - 1), "roots")
    out = bufs.output(out, (k, stride, SCALAR_BYTES), dev)
    if k:
        if _overlaps(out, r):
            raise ValueError("out overlaps the roots")
        _call("fr_poly_from_roots_segments", dev, r, seg, k, stride, out)
    return out


def fr_poly_quotients(coeffs, points, B, stride=None, out=None, ok=None):
    """Row j*B + i of the result: the B coefficients of coeffs[j](X) / (X - points[j][i]) followed by stride - B zeros (stride
    defaults to B); ok[j*B + i] = 1 iff the division is exact, otherwise the row is all zero.  coeffs: k x (B + 1) scalars,
    points: k x B (ints, uint8 arrays or CUDA tensors).  Returns (q [k*B, stride, 32], ok [k*B])."""
    if not isinstance(B, int) or not 1 <= B <= FR_POLY_MAX_B:
        raise ValueError("B must be in 1 .. %d (got %s)" % (FR_POLY_MAX_B, B))
    stride = B if stride is None else int(stride)
    if stride < B or stride > 1 << 24:                       # the C entries refuse the same range: sizes and row offsets stay far from overflow
        raise ValueError("stride must be in B .. 2^24 (got stride = %d, B = %d)" % (stride, B))
    coeffs, points = _fr_in(coeffs), _fr_in(points)
    dev = bufs.device_of(coeffs, points)
    p, k, _ = _fr_rows_arg(points, B, "points")
    c, nc = bufs.rows(coeffs, SCALAR_BYTES, "coeffs")
    if nc != k * (B + 1):
        raise ValueError("coeffs holds %d scalars, expected %d" % (nc, k * (B + 1)))
    out = bufs.output(out, (k * B, stride, SCALAR_BYTES), dev)
    ok = bufs.output(ok, (k * B,), dev, "ok")
    if k:
        _call("fr_poly_quotients", dev, c, p, B, k, stride, out, ok)
    return out, ok


def fr_lagrange_basis(set, B=None, nodes=None, m=None, x=None, out=None):
    """out[j][t] = prod over the elements s of set[j] with s != nodes[j][t] (mod r) of (x[j] - s) / (nodes[j][t] - s), for k rows:
    utils.ComputeLagrangeBasis with a node set per item (include/gpbc_bn254.h).  set: [rows][B] Python ints, or rows x B scalar
    rows (uint8 array / CUDA tensor) with B; nodes likewise with m, None = the set's own elements (m = B); x: scalars, None = 0.
    set and nodes have one row (shared by all) or k; x has one value or k; k is the largest of the three counts.  A set element
    equal to the node modulo r is skipped, so the result is total; a repeated element counts once per occurrence.
    Returns [k, m, 32] canonical scalars of the kind that went in (numpy, or a CUDA tensor)."""
    s, ns, B = _fr_rows_arg(set, B, "set")
    if nodes is None:
        if m is not None and int(m) != B:
            raise ValueError("without nodes m must equal B (got m = %s, B = %d)" % (m, B))
        nd, nn, m = None, ns, B
    else:
        nd, nn, m = _fr_rows_arg(nodes, m, "nodes")
    xs, nx = (None, 0) if x is None else bufs.rows(_fr_in(x), SCALAR_BYTES, "x")
    dev = bufs.device_of(s, nd, xs)
    k = max(ns, nn, nx)
    if ns not in (1, k) or nn not in (1, k) or (xs is not None and nx not in (1, k)):
        raise ValueError("set, nodes and x need one row or one row per output row (got %d, %d, %d)" % (ns, nn, nx))
    if k > (1 << 29) - 1:
        raise ValueError("too many rows for one call (%d)" % k)
    out = bufs.output(out, (k, m, SCALAR_BYTES), dev)
    if k:
        _call("fr_lagrange_basis", dev, s, ns, B, nd, nn, m, xs, nx, k, out)      # absent nodes / x go as null pointers
    return out


def fr_poly_eval(coeffs, points, d=None, m=None, out=None):
    """out[j][t] = sum_i coeffs[j][i] * points[j][t]^i modulo r for k rows: utils.ComputePolynomialValue, one polynomial and one point
    list per row (include/gpbc_bn254_share.h).  coeffs: [rows][d] Python ints, lowest degree first, or rows x d scalar rows (uint8 array /
    bytes / CUDA tensor) with d; points likewise with m.  Each has one row (shared by all) or k; k is the larger count.
    Returns [k, m, 32] canonical scalars of the kind that went in (numpy, or a CUDA tensor enqueued on the current stream)."""
    c, nc, d = _fr_rows_arg(coeffs, d, "coeffs")
    p, npts, m = _fr_rows_arg(points, m, "points")
    dev = bufs.device_of(c, p, out)
    k = max(nc, npts)
    if k and (nc not in (1, k) or npts not in (1, k)):
        raise ValueError("coeffs and points need one row or one row per output row (got %d, %d)" % (nc, npts))
    if k > (1 << 29) - 1:
        raise ValueError("too many rows for one call (%d)" % k)
    out = bufs.output(out, (k, m, SCALAR_BYTES), dev)
    if k:
        if _overlaps(out, c, p):
            raise ValueError("out overlaps an input")
        _call("fr_poly_eval", dev, c, nc, d, p, npts, m, k, out)
    return out


def _overlaps(out, *inputs):
    lo = bufs.address(out)
    hi = lo + bufs.nbytes(out)
    return any(x is not None and bufs.address(x) < hi and lo < bufs.address(x) + bufs.nbytes(x) for x in inputs)


SHARE_MAX = 1024
SHARE_ROOT = 0xFFFFFFFF


def _share_nodes(nodes, prefix=""):
    """a node list as a checked uint32 [n, 2] array; prefix ("tree 3: ") names the tree in a forest's messages"""
    try:
        arr = np.ascontiguousarray(np.asarray(nodes, dtype=np.int64).reshape(-1, 2))
    except (ValueError, TypeError):
        raise ValueError(prefix + "nodes must be a list of (parent, threshold) pairs") from None
    if arr.size and (arr.min() < 0 or arr.max() > SHARE_ROOT):
        raise ValueError(prefix + "parents and thresholds are unsigned 32-bit values")
    why = share_tree_check(arr.tolist())
    if why:
        raise ValueError("malformed " + (prefix or "tree: ") + why)
    return arr.astype(np.uint32)


def _share_counts(nodes):
    """(leaves, coefficients per item) of a checked node array"""
    return int((nodes[:, 1] == 0).sum()), int((nodes[:, 1].astype(np.int64) - 1)[nodes[:, 1] != 0].sum())


def _share_coeffs(coeffs, k, per_item, noun):
    """the coefficient argument of a share() as a byte buffer of k x per_item scalars, None where the tree / forest (noun) takes none"""
    if coeffs is not None and not bufs.is_torch(coeffs) and not isinstance(coeffs, (np.ndarray, bytes, bytearray)):
        coeffs = [v for row in coeffs for v in (row if isinstance(row, (list, tuple)) else [row])]
    if per_item:
        if coeffs is None:
            raise ValueError("the %s needs %d coefficients per item" % (noun, per_item))
        c, nc = bufs.rows(_fr_in(coeffs), SCALAR_BYTES, "coeffs")
        if nc != k * per_item:
            raise ValueError("coeffs holds %d scalars, expected %d x %d" % (nc, k, per_item))
        return c
    if coeffs is not None and bufs.nbytes(_fr_in(coeffs)):
        raise ValueError("the %s takes no coefficients" % noun)
    return None


class _ShareHandle:
    """what ShareTree and ShareForest do with their library handle: close() destroys it once, and so does the object's end"""
    _destroy = None

    def close(self):
        if self._h:
            getattr(self._lib, self._destroy)(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShareTree(_ShareHandle):
    """A threshold access tree uploaded once (include/gpbc_bn254_share.h): afterwards the shares of k secrets — AccessTreeNode.ShareSecret,
    the polynomial of every gate evaluated at its children's positions down to the leaves — are one launch.

        t = ShareTree(nodes)                     # nodes: [(parent, threshold)] in depth-first preorder; parent = SHARE_ROOT for node 0,
                                                 # threshold 0 = a leaf (bsw07.share_plan makes the list from a Leaf / Threshold tree)
        t.leaves, t.coeffs                       # L shares and C = sum of (threshold - 1) coefficients per item
        out = t.share(secrets, coeffs)           # secrets: k scalars, coeffs: [k, C] scalars (None when C == 0) -> [k, L, 32], leaf order
        w, ok = t.weights(held)                  # held: [k, L] bytes, non-zero = leaf held -> weights [k, L, 32] with sum w * share = secret, ok [k]

    Scalars are Python ints, uint8 arrays or CUDA tensors; CUDA tensors give a CUDA tensor enqueued on the current stream and not
    synchronised.  A malformed tree and every argument error are ValueError before the device is touched."""

    _destroy = "gpbc_share_tree_destroy"

    def __init__(self, nodes):
        self._h = ctypes.c_void_p()
        self.nodes = _share_nodes(nodes)
        self.leaves, self.coeffs = _share_counts(self.nodes)
        self._lib = _lib.load()
        _ensure_init()
        _lib.check(self._lib.gpbc_share_tree_create(self.nodes.ctypes.data, len(self.nodes), ctypes.byref(self._h)))
        assert (self.leaves, self.coeffs) == (self._lib.gpbc_share_tree_leaves(self._h), self._lib.gpbc_share_tree_coeffs(self._h))

    def share(self, secrets, coeffs=None, out=None):
        s, k = bufs.rows(_fr_in(secrets), SCALAR_BYTES, "secrets")
        c = _share_coeffs(coeffs, k, self.coeffs, "tree")
        dev = bufs.device_of(s, c, out)
        if k > (1 << 29) - 1:
            raise ValueError("too many items for one call (%d)" % k)
        out = bufs.output(out, (k, self.leaves, SCALAR_BYTES), dev)
        if not self._h:
            raise ValueError("the tree is closed")
        if k:
            if _overlaps(out, s, c):
                raise ValueError("out overlaps an input")
            _call("fr_share_tree", dev, self._h, s, c, k, out)
        return out

    def weights(self, held, out=None, ok_out=None):
        """(w [k, L, 32], ok [k]): the reconstruction weights of k attribute sets — AccessTreeNode.DecryptNode with the Lagrange
        coefficients multiplied down each leaf's path (include/gpbc_bn254_recon.h).  held: k x L bytes in leaf order, non-zero = the item
        holds the leaf's attribute (nested bools / ints, a uint8 or bool array, bytes, or a CUDA tensor).  A gate uses its first `threshold`
        satisfied children; every leaf that is not used gets 0; ok = 0 and a zero row where the root is not satisfied.  For ok = 1,
        sum_y w[y] share[y] is the secret for every output of share().  Outputs are of the kind that went in."""
        L = self.leaves
        hb, nheld = bufs.rows(_held_bytes(held, L), 1, "held")
        if nheld % L:
            raise ValueError("held holds %d bytes, not whole items of %d leaves" % (nheld, L))
        k = nheld // L
        dev = bufs.device_of(hb, out, ok_out)
        if k > (1 << 29) - 1:
            raise ValueError("too many items for one call (%d)" % k)
        out = bufs.output(out, (k, L, SCALAR_BYTES), dev)
        ok_out = bufs.output(ok_out, (k,), dev, "ok_out")
        if k:
            if _overlaps(out, hb, ok_out) or _overlaps(ok_out, hb):
                raise ValueError("an output overlaps the input or the other output")
            if not self._h:
                raise ValueError("the tree is closed")
            _call("fr_tree_weights", dev, self._h, hb, k, out, ok_out)
        return out, ok_out


FOREST_MAX_TREES = 65536


def _held_bytes(held, width):
    """held as ShareTree.weights takes it — nested bools / ints, a uint8 or bool array, bytes, or a CUDA tensor — as a flat byte buffer"""
    if isinstance(held, np.ndarray):
        if held.dtype not in (np.uint8, np.bool_):
            raise ValueError("held must be uint8 or bool (got %s)" % held.dtype)
        return held.astype(np.uint8, copy=False)
    if bufs.is_torch(held) or isinstance(held, (bytes, bytearray)):
        return held
    hrows = [list(h) for h in held]
    if any(len(h) != width for h in hrows):
        raise ValueError("held: every item needs %d entries" % width)
    return np.array([1 if v else 0 for h in hrows for v in h], dtype=np.uint8)


class ShareForest(_ShareHandle):
    """T threshold access trees uploaded once (include/gpbc_bn254_forest.h): afterwards the shares of k secrets, item i over the tree
    tree_of[i], are one launch, and so are the reconstruction weights of k attribute sets — ShareTree with a policy per item.

        f = ShareForest([nodes_0, nodes_1, ...])   # each a node list as ShareTree takes it
        f.trees, f.leaves, f.coeffs                # T, Lmax and Cmax: the columns of the per-item arrays
        f.tree_leaves, f.tree_coeffs               # [L_t], [C_t]
        out, ok = f.share(tree_of, secrets, coeffs)    # tree_of: k ids (uint32), coeffs: [k, Cmax] scalars, item i reads its first C_t
                                                       # -> [k, Lmax, 32] with the columns >= L_t zero; ok [k]: 1 where tree_of[i] < T
        w, ok = f.weights(tree_of, held)           # held: [k, Lmax] bytes, the columns >= L_t ignored -> [k, Lmax, 32], ok [k]:
                                                   # 0 where the root is unsatisfied OR the tree id is out of range (a zero row either way)

    Scalars are Python ints, uint8 arrays or CUDA tensors; tree_of is a list of ints, a uint32 array or an int32 CUDA tensor (the same
    bits).  CUDA tensors give CUDA tensors enqueued on the current stream and not synchronised.  A malformed tree and every argument error
    are ValueError before the device is touched."""

    _destroy = "gpbc_share_forest_destroy"

    def __init__(self, node_lists):
        self._h = ctypes.c_void_p()
        lists = list(node_lists)
        if not lists:
            raise ValueError("a forest needs at least one tree")
        if len(lists) > FOREST_MAX_TREES:
            raise ValueError("more than %d trees" % FOREST_MAX_TREES)
        arrays = [_share_nodes(nodes, "tree %d: " % t) for t, nodes in enumerate(lists)]
        self.nodes = np.ascontiguousarray(np.concatenate(arrays))
        self.node_off = np.cumsum([0] + [len(a) for a in arrays]).astype(np.uint32)
        self.trees = len(arrays)
        self.tree_leaves, self.tree_coeffs = (list(v) for v in zip(*map(_share_counts, arrays)))
        self.leaves, self.coeffs = max(self.tree_leaves), max(self.tree_coeffs)
        self._lib = _lib.load()
        _ensure_init()
        _lib.check(self._lib.gpbc_share_forest_create(self.nodes.ctypes.data, self.node_off.ctypes.data, self.trees, ctypes.byref(self._h)))
        assert (self.trees, self.leaves, self.coeffs) == (self._lib.gpbc_share_forest_trees(self._h), self._lib.gpbc_share_forest_leaves(self._h), self._lib.gpbc_share_forest_coeffs(self._h))
        assert all((L, C) == (self._lib.gpbc_share_forest_tree_leaves(self._h, t), self._lib.gpbc_share_forest_tree_coeffs(self._h, t))
                   for t, (L, C) in enumerate(zip(self.tree_leaves, self.tree_coeffs)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def _ids(tree_of):
        """(the k tree ids as a flat uint8 buffer of 4 k bytes, k): uint32 on the host, the same bits as int32 on the device"""
        if bufs.is_torch(tree_of):
            import torch
            if tree_of.dtype != torch.int32 or not tree_of.is_contiguous():
                raise ValueError("tree_of must be a contiguous int32 tensor (the bits of uint32 ids)")
            return tree_of.reshape(-1).view(torch.uint8), tree_of.numel()
        if isinstance(tree_of, np.ndarray):
            if tree_of.dtype != np.uint32:
                raise ValueError("tree_of must be uint32 (got %s)" % tree_of.dtype)
            ids = np.ascontiguousarray(tree_of).reshape(-1)
        else:
            ids = [int(t) for t in tree_of]
            if any(t < 0 or t > 0xFFFFFFFF for t in ids):
                raise ValueError("tree ids are unsigned 32-bit values")
            ids = np.array(ids, dtype=np.uint32)
        return ids.view(np.uint8), ids.size

    def share(self, tree_of, secrets, coeffs=None, out=None, ok_out=None):
        ids, k = self._ids(tree_of)
        s, ns = bufs.rows(_fr_in(secrets), SCALAR_BYTES, "secrets")
        if ns != k:
            raise ValueError("secrets holds %d scalars for %d tree ids" % (ns, k))
        c = _share_coeffs(coeffs, k, self.coeffs, "forest")
        dev = bufs.device_of(ids, s, c, out, ok_out)
        if k > (1 << 29) - 1:
            raise ValueError("too many items for one call (%d)" % k)
        out = bufs.output(out, (k, self.leaves, SCALAR_BYTES), dev)
        ok_out = bufs.output(ok_out, (k,), dev, "ok_out")
        if k:
            if _overlaps(out, ids, s, c, ok_out) or _overlaps(ok_out, ids, s, c):
                raise ValueError("an output overlaps an input or the other output")
            if not self._h:
                raise ValueError("the forest is closed")
            _call("fr_share_forest", dev, self._h, ids, s, c, k, out, ok_out)
        return out, ok_out

    def weights(self, tree_of, held, out=None, ok_out=None):
        """(w [k, Lmax, 32], ok [k]): ShareTree.weights with item i over the tree tree_of[i].  held: k x Lmax bytes, an item's first L_t
        columns in its tree's leaf order.  ok = 0 and a zero row where the root is not satisfied or the tree id is T or more."""
        L = self.leaves
        ids, k = self._ids(tree_of)
        hb, nheld = bufs.rows(_held_bytes(held, L), 1, "held")
        if nheld != k * L:
            raise ValueError("held holds %d bytes, expected %d x %d" % (nheld, k, L))
        dev = bufs.device_of(ids, hb, out, ok_out)
        if k > (1 << 29) - 1:
            raise ValueError("too many items for one call (%d)" % k)
        out = bufs.output(out, (k, L, SCALAR_BYTES), dev)
        ok_out = bufs.output(ok_out, (k,), dev, "ok_out")
        if k:
            if _overlaps(out, ids, hb, ok_out) or _overlaps(ok_out, ids, hb):
                raise ValueError("an output overlaps an input or the other output")
            if not self._h:
                raise ValueError("the forest is closed")
            _call("fr_forest_weights", dev, self._h, ids, hb, k, out, ok_out)
        return out, ok_out


def share_tree_check(nodes):
    """None, or why gpbc_share_tree_create would refuse the node list [(parent, threshold)] (the rules of include/gpbc_bn254_share.h)"""
    if not nodes:
        return "a tree needs at least one node"
    if nodes[0][0] != SHARE_ROOT:
        return "node 0 must carry the root marker"
    children, leaves, gates = [0] * len(nodes), 0, 0
    for i, (parent, threshold) in enumerate(nodes):
        if i:
            if parent == SHARE_ROOT:
                return "a second root"
            if parent >= i:
                return "a parent must come before its children"
            if not nodes[parent][1]:
                return "the parent of a node is a leaf"
            children[parent] += 1
        leaves, gates = leaves + (not threshold), gates + bool(threshold)
    if leaves > SHARE_MAX or gates > SHARE_MAX:
        return "more than %d leaves or %d gates" % (SHARE_MAX, SHARE_MAX)
    for (_, threshold), n in zip(nodes, children):
        if n > SHARE_MAX:
            return "more than %d children of one gate" % SHARE_MAX
        if threshold > n:
            return "a gate's threshold exceeds its number of children"
    return None


FR_LSSS_MAX = 64


def fr_lsss_weights(matrix, rows=None, cols=None, held=None, out=None, ok_out=None):
    """(w [k, rows, 32], ok [k]): for k systems the weights with sum_x w[x] M[x] = (1, 0, ..., 0) modulo r over the rows x whose
    byte in `held` is non-zero — FindLinearCombinationWeight with a policy per item (include/gpbc_bn254.h).  matrix: one
    rows x cols matrix (shared by the k masks) or k of them, as nested Python ints ([rows][cols] or [n][rows][cols]; rows and cols
    may then be omitted), a uint8 array or a CUDA tensor of 32-byte scalars; held: k x rows bytes (nested bools / ints, a uint8
    array or a CUDA tensor).  The used rows are the greedy first basis of the held rows; every other weight is 0; ok = 0 and a
    zero row where the held rows do not span the target.  Outputs are of the kind that went in (numpy, or CUDA tensors)."""
    if held is None:
        raise ValueError("held is required")
    if not bufs.is_torch(matrix) and not isinstance(matrix, (np.ndarray, bytes, bytearray)):
        m3 = [list(r) for r in matrix]
        if m3 and m3[0] and not isinstance(m3[0][0], (list, tuple)):
            m3 = [m3]                                                        # one [rows][cols] matrix
        m3 = [[list(r) for r in mat] for mat in m3]
        rows = len(m3[0]) if m3 and rows is None else rows
        cols = len(m3[0][0]) if m3 and m3[0] and cols is None else cols
        if any(len(mat) != rows or any(len(r) != cols for r in mat) for mat in m3):
            raise ValueError("matrix: every system needs %s rows of %s scalars" % (rows, cols))
        matrix = [v for mat in m3 for r in mat for v in r]
    for v, what in ((rows, "rows"), (cols, "cols")):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 1 <= int(v) <= FR_LSSS_MAX:
            raise ValueError("%s must be in 1 .. %d (got %s)" % (what, FR_LSSS_MAX, v))
    rows, cols = int(rows), int(cols)
    if isinstance(held, np.ndarray):
        if held.dtype not in (np.uint8, np.bool_):
            raise ValueError("held must be uint8 or bool (got %s)" % held.dtype)
        held = held.astype(np.uint8, copy=False)
    elif not bufs.is_torch(held) and not isinstance(held, (bytes, bytearray)):
        hrows = [list(h) for h in held]
        if any(len(h) != rows for h in hrows):
            raise ValueError("held: every mask needs %d entries" % rows)
        held = np.array([1 if v else 0 for h in hrows for v in h], dtype=np.uint8)
    matrix = _fr_in(matrix)
    dev = bufs.device_of(matrix, held)
    (mb, nscalars), (hb, nheld) = bufs.rows(matrix, SCALAR_BYTES, "matrix"), bufs.rows(held, 1, "held")
    if nscalars == 0 or nscalars % (rows * cols) or nheld % rows:
        raise ValueError("matrix needs whole systems of %d x %d scalars and held %d bytes per system" % (rows, cols, rows))
    nm, k = nscalars // (rows * cols), nheld // rows
    if nm not in (1, k):
        raise ValueError("need one matrix or one per mask (got %d matrices, %d masks)" % (nm, k))
    out = bufs.output(out, (k, rows, SCALAR_BYTES), dev)
    ok_out = bufs.output(ok_out, (k,), dev, "ok_out")
    if k:
        _call("fr_lsss_weights", dev, mb, nm, rows, cols, hb, k, out, ok_out)
    return out, ok_out


def fr_lsss_shares(matrix, vectors, rows=None, cols=None, out=None):
    """out[j][x] = sum_c matrix[j or 0][x][c] * vectors[j][c] modulo r, for k vectors: the shares lambda_x = M_x . v of
    LewkoWatersLsssMatrix.ComputeVector with v = (s, v_2, ..) per item (include/gpbc_bn254_indexed.h).  matrix: one rows x cols matrix
    (shared by the k vectors) or k of them, as nested Python ints ([rows][cols] or [n][rows][cols]; rows and cols may then be omitted), a
    uint8 array or a CUDA tensor of 32-byte scalars, in the layout fr_lsss_weights takes; vectors: [k][cols] ints or k x cols scalar rows.
    Entries are any value below 2^256 and act as their residue (-1 goes in as r - 1).  Returns [k, rows, 32] canonical scalars of the kind
    that went in (numpy, or a CUDA tensor enqueued on the current stream)."""
    if not bufs.is_torch(matrix) and not isinstance(matrix, (np.ndarray, bytes, bytearray)):
        m3 = [list(r) for r in matrix]
        if m3 and m3[0] and not isinstance(m3[0][0], (list, tuple)):
            m3 = [m3]                                                        # one [rows][cols] matrix
        m3 = [[list(r) for r in mat] for mat in m3]
        rows = len(m3[0]) if m3 and rows is None else rows
        cols = len(m3[0][0]) if m3 and m3[0] and cols is None else cols
        if any(len(mat) != rows or any(len(r) != cols for r in mat) for mat in m3):
            raise ValueError("matrix: every system needs %s rows of %s scalars" % (rows, cols))
        matrix = [v for mat in m3 for r in mat for v in r]
    for v, what in ((rows, "rows"), (cols, "cols")):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 1 <= int(v) <= FR_LSSS_MAX:
            raise ValueError("%s must be in 1 .. %d (got %s)" % (what, FR_LSSS_MAX, v))
    rows, cols = int(rows), int(cols)
    if not bufs.is_torch(vectors) and not isinstance(vectors, (np.ndarray, bytes, bytearray)):
        vrows = [list(r) for r in vectors]
        if any(len(r) != cols for r in vrows):
            raise ValueError("vectors: every vector needs %d scalars" % cols)
        vectors = [v for r in vrows for v in r]
    (mb, nscalars), (vb, nv) = bufs.rows(_fr_in(matrix), SCALAR_BYTES, "matrix"), bufs.rows(_fr_in(vectors), SCALAR_BYTES, "vectors")
    dev = bufs.device_of(mb, vb, out)
    if nscalars == 0 or nscalars % (rows * cols) or nv % cols:
        raise ValueError("matrix needs whole systems of %d x %d scalars and vectors %d scalars each" % (rows, cols, cols))
    nm, k = nscalars // (rows * cols), nv // cols
    if k and nm not in (1, k):
        raise ValueError("need one matrix or one per vector (got %d matrices, %d vectors)" % (nm, k))
    if k > (1 << 29) - 1:
        raise ValueError("too many vectors for one call (%d)" % k)
    out = bufs.output(out, (k, rows, SCALAR_BYTES), dev)
    if k:
        if _overlaps(out, mb, vb):
            raise ValueError("out overlaps an input")
        _call("fr_lsss_shares", dev, mb, nm, rows, cols, vb, k, out)
    return out


FR_SELECT_MAX = 1024


def fr_find_common(sets, lists, m, a, d, set_pos_out=None, list_pos_out=None, common_out=None, ok_out=None):
    """(set_pos [k, d], list_pos [k, d], common [k, d, 32], ok [k]): utils.FindCommonAttributes for k items in one launch
    (include/gpbc_bn254_select.h).  lists: k x a scalar rows, the attributes of k ciphertexts; sets: m scalar rows (one key for all items)
    or k x m (a key per item).  Rows are 32-byte little-endian values below 2^256, compared modulo r; uint8 arrays or CUDA tensors,
    not mixed.  Per item the list is walked in order and an element is kept iff the set holds it and no earlier equal element was
    kept, up to d: slot s of the rows is the s-th kept element's position in the set (its first occurrence there), its position in the
    list and its canonical value — `common` is the node set fr_lagrange_basis takes.  ok = 0 and all-zero rows where fewer than d are
    kept.  The positions come back as int32; a caller's set_pos_out / list_pos_out are uint8 buffers of k x d x 4 bytes, 4-byte aligned.
    Outputs are of the kind that went in; tensors are enqueued on the current stream and not synchronised."""
    for v, what in ((m, "m"), (a, "a"), (d, "d")):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 1 <= int(v) <= FR_SELECT_MAX:
            raise ValueError("%s must be in 1 .. %d (got %s)" % (what, FR_SELECT_MAX, v))
    m, a, d = int(m), int(a), int(d)
    for v, what in ((sets, "sets"), (lists, "lists")):
        if not bufs.is_torch(v) and not isinstance(v, (np.ndarray, bytes, bytearray)):
            raise ValueError("%s must be a uint8 array or a CUDA tensor of 32-byte rows (sw05.attribute_rows makes them from integers)" % what)
        if isinstance(v, np.ndarray) and v.dtype != np.uint8:
            raise ValueError("%s must be uint8 (got %s)" % (what, v.dtype))
    (sb, ns), (lb, nl) = bufs.rows(sets, SCALAR_BYTES, "sets"), bufs.rows(lists, SCALAR_BYTES, "lists")
    outs = (set_pos_out, list_pos_out, common_out, ok_out)
    dev = bufs.device_of(sb, lb, *outs)
    if ns == 0 or ns % m or nl % a:
        raise ValueError("sets needs whole sets of %d scalars and lists whole lists of %d" % (m, a))
    n_sets, k = ns // m, nl // a
    if k and n_sets not in (1, k):
        raise ValueError("need one set or one per list (got %d sets, %d lists)" % (n_sets, k))
    if k > (1 << 29) - 1:
        raise ValueError("too many items for one call (%d)" % k)
    sp = bufs.output(set_pos_out, (k, d, 4), dev, "set_pos_out")
    lp = bufs.output(list_pos_out, (k, d, 4), dev, "list_pos_out")
    cm = bufs.output(common_out, (k, d, SCALAR_BYTES), dev, "common_out")
    ok = bufs.output(ok_out, (k,), dev, "ok_out")
    if bufs.address(sp) % 4 or bufs.address(lp) % 4:
        raise ValueError("set_pos_out and list_pos_out must be 4-byte aligned")
    if k:
        got = (sp, lp, cm, ok)
        if any(_overlaps(o, sb, lb, *got[:i]) for i, o in enumerate(got)):
            raise ValueError("an output overlaps an input or another output")
        _call("fr_find_common", dev, sb, n_sets, m, lb, a, d, k, sp, lp, cm, ok)

    def positions(x):
        if bufs.is_torch(x):
            import torch
            return x.reshape(-1).view(torch.int32).reshape(k, d)
        return x.reshape(-1).view(np.int32).reshape(k, d)
    return positions(sp), positions(lp), cm.reshape(k, d, SCALAR_BYTES), ok.reshape(k)


FORMULA_MAX_NODES = 127


def _formula_nodes(nodes):
    """(buffer, number of formulas, n_nodes) of an int64 array or CUDA tensor [k, N] (or [N]: one formula) of formula codes"""
    if bufs.is_torch(nodes):
        if str(nodes.dtype) != "torch.int64" or not nodes.is_contiguous():
            raise ValueError("nodes must be a contiguous int64 tensor")
    elif isinstance(nodes, np.ndarray):
        if nodes.dtype != np.int64:
            raise ValueError("nodes must be int64 (got %s)" % nodes.dtype)
        nodes = np.ascontiguousarray(nodes)
    else:
        raise ValueError("nodes must be an int64 array or a CUDA tensor of formula codes (formula.encode makes them)")
    if nodes.ndim not in (1, 2) or not 1 <= nodes.shape[-1] <= FORMULA_MAX_NODES:
        raise ValueError("nodes must be [k, N] or [N] with N in 1 .. %d (got shape %s)" % (FORMULA_MAX_NODES, tuple(nodes.shape)))
    return nodes, (1 if nodes.ndim == 1 else int(nodes.shape[0])), int(nodes.shape[-1])


def _formula_size(v, what):
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 1 <= int(v) <= FR_LSSS_MAX:
        raise ValueError("%s must be in 1 .. %d (got %s)" % (what, FR_LSSS_MAX, v))
    return int(v)


def _typed(x, dtype, *shape):
    """a uint8 output buffer as its typed view"""
    if bufs.is_torch(x):
        import torch
        return x.reshape(-1).view(getattr(torch, dtype)).reshape(*shape)
    return x.reshape(-1).view(getattr(np, dtype)).reshape(*shape)


def fr_lsss_from_formula(nodes, rows, cols, matrix_out=None, rho_out=None, dims_out=None, ok_out=None):
    """(matrix [k, rows, cols, 32], rho [k, rows] int64, dims [k, 2] int32, ok [k]): the Lewko-Waters share matrices of k boolean
    formulas in one launch — NewLSSSMatrixFromBinaryTree per item (include/gpbc_bn254_formula.h).  nodes: [k, N] int64 codes, a numpy
    array or a CUDA tensor (formula.encode makes them): a tree in preorder, a code >= 0 a leaf with that attribute, -2 AND, -3 OR, -1
    padding behind the tree.  The matrix is in the layout fr_lsss_shares and fr_lsss_weights read: entries 0, 1 and r - 1, rows and
    columns past an item's own all zero, rho there -1; dims is the item's own (rows, columns).  ok = 0 with a zero matrix, rho all -1 and
    dims (0, 0) for a malformed formula, more leaves than `rows` or more columns than `cols`.  A caller's outputs are uint8 buffers of
    k x rows x cols x 32, k x rows x 8 (8-byte aligned), k x 2 x 4 (4-byte aligned) and k bytes.  Outputs are of the kind that went in;
    tensors are enqueued on the current stream and not synchronised."""
    rows, cols = _formula_size(rows, "rows"), _formula_size(cols, "cols")
    nodes, k, N = _formula_nodes(nodes)
    outs = (matrix_out, rho_out, dims_out, ok_out)
    dev = bufs.device_of(nodes, *outs)
    if k > (1 << 29) - 1:
        raise ValueError("too many items for one call (%d)" % k)
    mat = bufs.output(matrix_out, (k, rows, cols, SCALAR_BYTES), dev, "matrix_out")
    rho = bufs.output(rho_out, (k, rows, 8), dev, "rho_out")
    dims = bufs.output(dims_out, (k, 2, 4), dev, "dims_out")
    ok = bufs.output(ok_out, (k,), dev, "ok_out")
    if bufs.address(rho) % 8 or bufs.address(dims) % 4:
        raise ValueError("rho_out must be 8-byte aligned and dims_out 4-byte aligned")
    if k:
        got = (mat, rho, dims, ok)
        nb = _typed(nodes, "uint8", -1)
        if any(_overlaps(o, nb, *got[:i]) for i, o in enumerate(got)):
            raise ValueError("an output overlaps the input or another output")
        _call("fr_lsss_from_formula", dev, nodes, N, k, rows, cols, mat, rho, dims, ok)
    return mat.reshape(k, rows, cols, SCALAR_BYTES), _typed(rho, "int64", k, rows), _typed(dims, "int32", k, 2), ok.reshape(k)


def formula_select(nodes, held, rows, chosen_out=None, ok_out=None):
    """(chosen [k, rows], ok [k]): for k keys the leaves of a formula whose rows recombine with weight 1 (include/gpbc_bn254_formula.h).
    nodes: [k, N] int64 codes, or [N] / [1, N] for one formula shared by all keys; held: k x rows bytes in leaf order, the mask
    fr_lsss_weights takes on the matrix of fr_lsss_from_formula.  From a satisfied root both children of an AND are taken and, at an OR,
    the left child if it is satisfied, else the right; chosen is 1 at the leaves reached.  ok = 0 and a zero row for an unsatisfied root,
    a malformed formula or more leaves than `rows`.  For ok = 1 the chosen rows of the matrix sum to (1, 0, ..., 0).  Outputs are of the
    kind that went in; tensors are enqueued on the current stream and not synchronised."""
    rows = _formula_size(rows, "rows")
    nodes, nf, N = _formula_nodes(nodes)
    if isinstance(held, np.ndarray):
        if held.dtype not in (np.uint8, np.bool_):
            raise ValueError("held must be uint8 or bool (got %s)" % held.dtype)
        held = held.astype(np.uint8, copy=False)
    elif not bufs.is_torch(held):
        raise ValueError("held must be a uint8 array or a CUDA tensor")
    hb, nheld = bufs.rows(held, 1, "held")
    dev = bufs.device_of(nodes, hb, chosen_out, ok_out)
    if nheld % rows:
        raise ValueError("held needs %d bytes per item" % rows)
    k = nheld // rows
    if k and nf not in (1, k):
        raise ValueError("need one formula or one per mask (got %d formulas, %d masks)" % (nf, k))
    if k > (1 << 29) - 1:
        raise ValueError("too many items for one call (%d)" % k)
    chosen = bufs.output(chosen_out, (k, rows), dev, "chosen_out")
    ok = bufs.output(ok_out, (k,), dev, "ok_out")
    if k:
        nb = _typed(nodes, "uint8", -1)
        if _overlaps(chosen, nb, hb) or _overlaps(ok, nb, hb, chosen):
            raise ValueError("an output overlaps an input or the other output")
        _call("formula_select", dev, nodes, nf, N, hb, k, rows, chosen, ok)
    return chosen.reshape(k, rows), ok.reshape(k)


_gen_tables = {}


def _scalar_mul_base(g2, scalars):
    """Small host-side calls go through fixed-base window tables of the generator (built on the first call, kept until shutdown():
    32 mixed additions per multiplication instead of the variable-base kernel's doublings — what include/gpbc_bn254.hpp and the Go
    shim do); large batches and device tensors take the shared-base form of the variable-base kernel, which builds its own table."""
    k, n = bufs.rows(scalars_to_bytes(scalars), SCALAR_BYTES, "scalars")
    gen = generators()[1 if g2 else 0]
    if bufs.is_torch(k) or n >= 16384:
        return (g2_scalar_mul if g2 else g1_scalar_mul)(bufs.put(gen, k), k)
    _ensure_init()
    if g2 not in _gen_tables:
        _gen_tables[g2] = FixedBase(gen, g2=g2)
    return _gen_tables[g2].mul(k)


def g1_scalar_mul_base(scalars):
    """ScalarMultiplicationBase: [s]g1."""
    return _scalar_mul_base(False, scalars)


def g2_scalar_mul_base(scalars):
    return _scalar_mul_base(True, scalars)


def _sum(group, width, pts):
    dev = bufs.device_of(pts)
    pts, n = bufs.rows(pts, width, "points")
    out = bufs.output(None, (1, width), dev)
    # only the device form takes a caller-side workspace (the host form stages through the library's own)
    ws = () if dev is None else _workspace(None, _lib.load().gpbc_sum_workspace_bytes(n, int(group == "g2")), dev)
    _call(group + "_sum", dev, pts, n, out, *ws)
    return out[0]


def g1_sum(pts):
    """Sum of affine G1 points (chains of G1Affine.Add in the reference)."""
    return _sum("g1", G1_BYTES, pts)


def g2_sum(pts):
    return _sum("g2", G2_BYTES, pts)


def _scalar_mul_sum(group, width, bases, scalars):
    scalars = scalars_to_bytes(scalars)
    dev = bufs.device_of(bases, scalars)
    (bases, nbase), (scalars, n) = bufs.rows(bases, width, "bases"), bufs.rows(scalars, SCALAR_BYTES, "scalars")
    if nbase != n:
        raise ValueError("need one base per scalar")
    out = bufs.output(None, (1, width), dev)
    _call(group + "_scalar_mul_sum", dev, bases, scalars, n, out)
    return out[0]


def g1_scalar_mul_sum(bases, scalars):
    """sum_i [s_i] P_i (the verifier's sums of BLS aggregate verification, BASELINE config 3).  Host buffers: sharded over the
    bound devices.  CUDA tensors: this rank's shard; with a communicator (comm_init_rank) the result is the sum over ALL
    ranks — one RCCL all-gather of a point per rank inside the library."""
    return _scalar_mul_sum("g1", G1_BYTES, bases, scalars)


def g2_scalar_mul_sum(bases, scalars):
    return _scalar_mul_sum("g2", G2_BYTES, bases, scalars)


# --------------------------------------------------------------------------------------- collectives (RCCL inside the library)
COMM_ID_BYTES = 128


def comm_init_all():
    """One RCCL communicator over all bound devices of this process (rank = device slot)."""
    _ensure_init()
    _lib.check(_lib.load().gpbc_comm_init_all())


def comm_unique_id():
    """128 opaque bytes from rank 0, to be handed to every rank's comm_init_rank (any transport: torch.distributed
    broadcast, a file, the launcher's environment)."""
    ident = (ctypes.c_uint8 * COMM_ID_BYTES)()
    _lib.check(_lib.load().gpbc_comm_get_unique_id(ident))
    return bytes(ident)


def comm_init_rank(unique_id, n_ranks, rank):
    """Join the multi-process communicator as `rank` with this process's current device (one process per GPU)."""
    if len(unique_id) != COMM_ID_BYTES:
        raise ValueError("the communicator id is %d bytes" % COMM_ID_BYTES)
    _ensure_init()
    ident = (ctypes.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
    _lib.check(_lib.load().gpbc_comm_init_rank(ident, int(n_ranks), int(rank)))


def comm_ranks():
    return int(_lib.load().gpbc_comm_ranks())


def comm_destroy():
    _lib.check(_lib.load().gpbc_comm_destroy())


def allgather(send, out=None):
    """All-gather equal-sized uint8 CUDA blocks over the library's communicator: returns [n_ranks, send.numel()].
    Enqueued on the current torch stream, not synchronised."""
    dev = bufs.device_of(send)
    if dev is None:
        raise ValueError("send must be a CUDA tensor: the collective runs between devices")
    send, nb = bufs.rows(send, 1, "send")
    _ensure_init()
    ranks = comm_ranks()
    if ranks < 1:
        raise EngineError("no communicator: call comm_init_rank() / comm_init_all() first")
    out = bufs.output(out, (ranks, nb), dev)
    _call("allgather", dev, send, nb, out)
    return out


# --------------------------------------------------------------------------------------- GT
def gt_exp(x, k, out=None):
    """out[i] = new(GT).Exp(x[i], k[i]); Python ints may be negative (inverse, as gnark)."""
    if isinstance(k, int):
        k = [k]
    if isinstance(k, (list, tuple)):
        neg = [i for i, s in enumerate(k) if int(s) < 0]
        if neg:
            x = bufs.copy(bufs.view(x, -1, GT_BYTES))                     # the caller's bases stay as they are
            x[neg] = gt_inverse(bufs.take(x, neg))
        k = np.frombuffer(b"".join(abs(int(s)).to_bytes(32, "little") for s in k), dtype=np.uint8)
    if bufs.is_torch(x) and not bufs.is_torch(k):
        k = bufs.put(bufs.rows(k, SCALAR_BYTES, "k")[0].copy(), x)        # device bases with a host exponent list
    return _rowwise("gt_exp_batch", GT_BYTES, (x, GT_BYTES, "x"), (k, SCALAR_BYTES, "k"), out=out)


def gt_multi_exp(x, k, seg_off, out=None, workspace=None):
    """out[s] = prod_{i in [seg_off[s], seg_off[s+1])} x[i]^k[i]: the `res.Mul(res, tmp.Exp(c, w))` loops of the reference as one call,
    every factor with GT.Exp's semantics (256-bit exponents as they are, any Fp12 base), the squarings shared by four factors.
    k: one exponent per element, or ONE list of m exponents when every segment has exactly m elements (the weights of a policy
    against many ciphertexts), or None for the plain product; Python ints must be in [0, 2^256).  numpy arrays in, numpy array out;
    CUDA tensors in (seg_off a host sequence, or an int64 / uint64 CUDA tensor that is then validated on the device), CUDA tensor
    out, enqueued on the current torch stream.  Arguments are checked before the engine is touched."""
    op = _SegRed("gt_multi_exp", GT_BYTES, "x", "k", "elements", "one exponent per element", "exponent",
                 "exponents must be in [0, 2^256): invert the base for a negative one", lambda lib, n, n_seg: lib.gpbc_gt_multi_exp_workspace_bytes(n, n_seg), 1)
    return _segmented_reduce(op, x, k, seg_off, out, workspace)


def gt_prod(x, seg_off=None):
    """Products in GT without exponents: out[s] = prod x[seg_off[s]:seg_off[s+1]] (the GT sibling of g1_sum — the chain of GT.Mul in
    `AggregatePublicKeys`); without seg_off the product of all of x as ONE element."""
    if seg_off is None:
        return gt_multi_exp(x, None, [0, bufs.nbytes(x) // GT_BYTES])[0]
    return gt_multi_exp(x, None, seg_off)


def gt_mul(a, b):
    return _rowwise("gt_mul_batch", GT_BYTES, (a, GT_BYTES, "a"), (b, GT_BYTES, "b"))


def gt_div(a, b):
    return _rowwise("gt_div_batch", GT_BYTES, (a, GT_BYTES, "a"), (b, GT_BYTES, "b"))


def gt_inverse(a):
    return _rowwise("gt_inverse_batch", GT_BYTES, (a, GT_BYTES, "a"))


def gt_equal(a, b, out=None):
    """ok[i] = 1 where a[i] == b[i] (or == b[0] for a single b), else 0: (*GT).Equal per row, the 384 bytes compared as they are
    (include/gpbc_bn254_verify.h).  uint8 [n] of the kind the inputs are: the verdicts of a device-resident batch stay in HBM.  An
    empty batch returns an empty result without touching the engine."""
    dev = bufs.device_of(a, b)
    (a, n), (b, nb) = bufs.rows(a, GT_BYTES, "a"), bufs.rows(b, GT_BYTES, "b")
    if nb not in (1, n):
        raise ValueError("need one b or one b per a (got %d for %d)" % (nb, n))
    out = bufs.output(out, (n,), dev)
    if n:
        _call("gt_equal", dev, a, b, nb, n, out)
    return out


# --------------------------------------------------------------------------------------- membership of in-memory elements
# (*G1Affine|*G2Affine).IsOnCurve / IsInSubGroup and (*GT).IsInSubGroup for n structs as they are in memory
# (include/gpbc_bn254_member.h): what guards elements that did not come through g1_unmarshal / g2_unmarshal — the only other places where
# the engine validates anything.
def _member(name, width, x, out):
    """ok[i] = the verdict for row i: uint8 [n] of the kind `x` is.  An empty batch returns an empty result without touching the engine."""
    dev = bufs.device_of(x, out)
    x, n = bufs.rows(x, width, "x")
    out = bufs.output(out, (n,), dev)
    if n:
        _call(name, dev, x, n, out)
    return out


def g1_is_on_curve(x, out=None):
    """ok[i] = 1 where the G1Affine struct x[i] is on the curve (the point at infinity is), else 0; a coordinate whose stored value is not
    below p gives 0.  Host arrays in, host array out; CUDA tensors in, CUDA tensor out on the current stream."""
    return _member("g1_is_on_curve", G1_BYTES, x, out)


g1_is_in_subgroup = g1_is_on_curve           # the cofactor of G1 is 1: gnark's IsInSubGroup is the same verdict


def g2_is_on_curve(x, out=None):
    """ok[i] = 1 where the G2Affine struct x[i] is on the twist (infinity is), else 0"""
    return _member("g2_is_on_curve", G2_BYTES, x, out)


def g2_is_in_subgroup(x, out=None):
    """ok[i] = 1 where x[i] is on the twist AND in its subgroup of order r (gnark's endomorphism identity), else 0.  gnark's IsInSubGroup
    evaluates the identity without a curve test; this entry's 0 for a point off the twist is the project's definition."""
    return _member("g2_is_in_subgroup", G2_BYTES, x, out)


def gt_is_in_subgroup(x, out=None):
    """ok[i] = 1 where the GT struct x[i] is canonical, not zero and of order dividing r (cyclotomic and x^p == x^(6u^2): gnark's
    E12.IsInSubGroup, which read literally accepts zero; this entry does not), else 0"""
    return _member("gt_is_in_subgroup", GT_BYTES, x, out)


def fp_mul(a, b):
    """Batched Fp Montgomery product (kernel unit test entry; host buffers only)."""
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    return _rowwise("fp_mul_batch", 32, (a, 32, "a"), (b, 32, "b"))


# --------------------------------------------------------------------------------------- wire formats
# gnark Marshal()/RawBytes(), Bytes() and Unmarshal()/SetBytes() (reference serialization/serialization_curve.go:5-33,
# ibe/gentry06_ibe/gentry06_ibe.go:322-324, hash/hash_from_gt.go:5-8), batched.  Encodings are rows of
# 64 / 32 (G1), 128 / 64 (G2) and 384 (GT) big-endian canonical bytes.
_WIRE = {"g1": (G1_BYTES, 64, 32), "g2": (G2_BYTES, 128, 64), "gt": (GT_BYTES, 384, 384)}


def _marshal(kind, x, compressed):
    mem, raw, comp = _WIRE[kind]
    dev = bufs.device_of(x)
    x, n = bufs.rows(x, mem, kind + " elements")
    out = bufs.output(None, (n, comp if compressed else raw), dev)
    cflag = () if kind == "gt" else (1 if compressed else 0,)
    _call(kind + "_marshal_batch", dev, x, n, *cflag, out)
    return out


def _unmarshal(kind, enc, elem_bytes):
    mem, raw, comp = _WIRE[kind]
    if elem_bytes is None:
        elem_bytes = raw
    if elem_bytes not in (raw, comp):
        raise ValueError("%s element size must be %d or %d" % (kind, comp, raw))
    dev = bufs.device_of(enc)
    enc, n = bufs.rows(enc, elem_bytes, kind + " encodings")
    out, ok = bufs.output(None, (n, mem), dev), bufs.output(None, (n,), dev)
    width = () if kind == "gt" else (elem_bytes,)
    _call(kind + "_unmarshal_batch", dev, enc, *width, n, out, ok)
    return out, ok


def g1_marshal(pts, compressed=False):
    """G1Affine.Marshal() (64 B rows) or, compressed, G1Affine.Bytes() (32 B rows)."""
    return _marshal("g1", pts, compressed)


def g2_marshal(pts, compressed=False):
    """G2Affine.Marshal() (128 B rows) or, compressed, G2Affine.Bytes() (64 B rows)."""
    return _marshal("g2", pts, compressed)


def gt_marshal(gt):
    """GT.Marshal() = GT.Bytes(): 384 B rows, coefficients C1.B2.A1 ... C0.B0.A0."""
    return _marshal("gt", gt, False)


def g1_unmarshal(buf, elem_bytes=None):
    """G1Affine.Unmarshal() on rows of `elem_bytes` (64 default, or 32): (points, ok).  ok[i] = 0 where gnark returns an
    error (the point row is then zero); the reference drops that error, callers here should look at it."""
    return _unmarshal("g1", buf, elem_bytes)


def g2_unmarshal(buf, elem_bytes=None):
    """G2Affine.Unmarshal() on rows of `elem_bytes` (128 default, or 64): (points, ok); includes the subgroup check."""
    return _unmarshal("g2", buf, elem_bytes)


def gt_unmarshal(buf):
    """GT.Unmarshal(): (values, ok)."""
    return _unmarshal("gt", buf, None)


# --------------------------------------------------------------------------------------- hash to curve, group part
def map_to_g1(u):
    """Tail of bn254.HashToG1: rows of two fp.Element (64 B, gnark layout) -> MapToCurve1(u0) + MapToCurve1(u1)."""
    return _rowwise("g1_map_to_curve_batch", G1_BYTES, (u, G1_BYTES, "field elements"))


def map_to_g2(u):
    """Tail of bn254.HashToG2: rows of two E2 (128 B) -> ClearCofactor(MapToCurve2(u0) + MapToCurve2(u1))."""
    return _rowwise("g2_map_to_curve_batch", G2_BYTES, (u, G2_BYTES, "field elements"))


def _messages(msgs, msg_off):
    """(dev, data, msg_off, nbytes, n) of the entries that take n messages.  msgs: a list of bytes-like messages (host), or the
    concatenated bytes as a numpy array / CUDA uint8 tensor with msg_off (n + 1 offsets; numpy uint64 for host data, an int64 CUDA
    tensor for device data).  nbytes: the arguments the device form takes besides — the length of the message buffer — as a tuple."""
    if bufs.is_torch(msgs):
        # The three message forms are the reason this body names the buffer kind: the device form takes its offsets as an int64
        # tensor and the length of the message buffer besides.
        dev = bufs.device_of(msgs, msg_off)
        if dev is None or msg_off is None or str(msg_off.dtype) != "torch.int64" or not msg_off.is_contiguous():
            raise ValueError("device messages need msg_off as a contiguous int64 tensor on the same device")
        msgs, nbytes = bufs.rows(msgs, 1, "messages")
        n = msg_off.numel() - 1
        if n < 0:
            raise ValueError("msg_off needs n + 1 entries")
        return dev, msgs, msg_off, (nbytes,), n
    if msg_off is None:
        msgs = [bytes(m) for m in msgs]
        msg_off = np.zeros(len(msgs) + 1, dtype=np.uint64)
        if msgs:
            msg_off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
        data = np.frombuffer(b"".join(msgs), dtype=np.uint8) if msgs and int(msg_off[-1]) else np.zeros(1, dtype=np.uint8)
    else:
        data = np.ascontiguousarray(np.asarray(msgs, dtype=np.uint8)).reshape(-1)
        msg_off = np.ascontiguousarray(np.asarray(msg_off, dtype=np.uint64))
        if msg_off.size < 1 or (msg_off.size > 1 and int(msg_off[-1]) > data.size):
            raise ValueError("message offsets exceed the message buffer")
        if data.size == 0:
            data = np.zeros(1, dtype=np.uint8)
    return None, data, msg_off, (), msg_off.size - 1


def _hash_messages(what, msgs, dst, msg_off=None):
    """Shared body of hash_to_g1 / hash_to_g2 / hash_to_field.  what: 0 G1, 1 G2, 2 / 4 field elements per message; the messages as
    _messages takes them."""
    dst = bytes(dst)
    if len(dst) > 255:                                           # gnark's ExpandMsgXmd refuses it ("invalid domain size"), so does the Go shim
        raise ValueError("invalid domain size (>255 bytes)")
    width = G1_BYTES if what == 0 else G2_BYTES if what == 1 else 32 * what
    name = ("hash_to_g1", "hash_to_g2", "hash_to_field")[min(what, 2)]
    dbuf = ctypes.create_string_buffer(dst, len(dst) if dst else 1)
    count = (what,) if what >= 2 else ()
    dev, data, msg_off, nbytes, n = _messages(msgs, msg_off)
    out = bufs.output(None, (n, width), dev)
    if n or dev is not None:
        _call(name, dev, data, msg_off, *nbytes, n, dbuf, len(dst), *count, out)
    return out


def hash_to_g1(msgs, dst, msg_off=None):
    """bn254.HashToG1(msg, dst) for every message, hashing included (expand_message_xmd with SHA-256 on the device)."""
    return _hash_messages(0, msgs, dst, msg_off)


def hash_to_g2(msgs, dst, msg_off=None):
    """bn254.HashToG2(msg, dst) for every message, hashing included."""
    return _hash_messages(1, msgs, dst, msg_off)


def hash_to_field(msgs, dst, count=2, msg_off=None):
    """fp.Hash(msg, dst, count) for every message: [n, count * 32] fp.Elements in gnark's layout (count = 2 or 4)."""
    if count not in (2, 4):
        raise ValueError("count must be 2 or 4")
    return _hash_messages(count, msgs, dst, msg_off)


# --------------------------------------------------------------------------------------- SHA-256 with the digest as bytes or as a scalar
def sha256(msgs, msg_off=None, to_fr=False, out=None):
    """SHA-256 of every message on the device (include/gpbc_bn254_hash.h): [n, 32] digests as SHA-256 writes them — the identity masks
    of NewWaters05IBEIdentity — or, with to_fr, fr.Element.SetBytes(digest) in the scalar format (little-endian, canonical).  The
    messages as hash_to_field takes them: a list of bytes, or a flat buffer plus offsets, host or CUDA."""
    dev, data, msg_off, nbytes, n = _messages(msgs, msg_off)
    out = bufs.output(out, (n, 32), dev)
    if n or dev is not None:
        _call("sha256_batch", dev, data, msg_off, *nbytes, n, 1 if to_fr else 0, out)
    return out


def hash_g1_gt_gt_to_fr(u, v, w, out=None):
    """beta = H(u, v, w) of Gentry06 (ibe/gentry06_ibe/gentry06_ibe.go:319-343) for n items: fr.SetBytes(SHA-256(u.Bytes() ||
    v.Bytes() || w.Bytes())) with u [n, 64] G1 points and v, w [n, 384] GT elements -> [n, 32] scalars, canonical.  One launch; the
    800 bytes are never written.  The output is of the kind the inputs are."""
    return _rowwise("hash_g1_gt_gt_to_fr", SCALAR_BYTES, (u, G1_BYTES, "u"), (v, GT_BYTES, "v"), (w, GT_BYTES, "w"), out=out)


# --------------------------------------------------------------------------------------- the XOR mask from GT bytes
def gt_xor_mask(gt, msgs, msg_off=None, out=None):
    """(out, out_len): out_i = msg_i XOR GT.Bytes()(gt_i) cut to the shorter of the two — utils.Xor(message, hash.FromGT(gid)), the last
    step of Boneh-Franklin Encrypt and Decrypt (ibe/bf01_ibe/bf01_ibe.go:170-176,202-208; include/gpbc_bn254_mask.h) — for n items in ONE
    launch.  gt: [n, 384] GT elements.  The messages as sha256 takes them, plus a row form:
        a list of bytes (host)                                         out is (flat uint8 array, uint64 offsets [n + 1])
        a flat buffer plus msg_off (numpy uint64 / an int64 CUDA tensor)    out is a flat buffer of the message buffer's size
        an [n, width] uint8 array or CUDA tensor, msg_off=None         out is [n, width]
    out_len [n] = min(len_i, 384), the length of the slice the reference returns (uint32 on the host, the same bits as int32 on the
    device); out[L_i:len_i] is zero.  The output is of the kind the inputs are.  `out` may be given — it has the layout of the message
    buffer — and may be the message buffer itself: the call then runs in place.  Bytes of a given `out` that belong to no message are
    left as they are; in a buffer made here they are undefined."""
    if bufs.is_torch(gt) != bufs.is_torch(msgs):
        raise ValueError("the GT elements and the messages must both be host data or both CUDA tensors")
    if msg_off is None and not isinstance(msgs, (list, tuple)):
        if not (isinstance(msgs, np.ndarray) or bufs.is_torch(msgs)) or msgs.ndim != 2:
            raise ValueError("messages without msg_off are a list of bytes or an [n, width] uint8 array / tensor")
        dev = bufs.device_of(gt, msgs, out)
        n, width = (int(e) for e in msgs.shape)
        data, off, shape = bufs.rows(msgs, 1, "messages")[0], None, (n, width)
        nbytes = () if dev is None else (n * width,)
    else:
        dev, data, off, nbytes, n = _messages(msgs, msg_off)
        bufs.device_of(gt, data, out)
        # (_messages hands an empty host buffer on as one byte, so that it has an address; the output is of the true size)
        size = bufs.nbytes(data) if dev is not None else int(off[-1]) if isinstance(msgs, (list, tuple)) else np.asarray(msgs).size
        width, shape = 0, (size,)
    gt, ng = bufs.rows(gt, GT_BYTES, "gt")
    if ng != n:
        raise ValueError("%d GT elements for %d messages" % (ng, n))
    given = out
    out = bufs.output(out, shape, dev)
    out_len = bufs.output(None, (n, 4), dev)
    if given is not None and bufs.address(out) != bufs.address(data) and _overlaps(out, data):
        raise ValueError("out overlaps the messages (only the message buffer itself runs in place)")
    if given is not None and _overlaps(out, gt):
        raise ValueError("out overlaps gt")
    if n:
        _call("gt_xor_mask", dev, gt, data, off, *nbytes, width, n, out, out_len)
    if dev is None:
        out_len = out_len.view(np.uint32).reshape(n)
    else:
        import torch
        out_len = out_len.view(torch.int32).reshape(n)
    if isinstance(msgs, (list, tuple)):
        return (out, off), out_len
    return out, out_len


# --------------------------------------------------------------------------------------- randomness addressed by (seed, stream, index)
RANDOM_SEED_BYTES = 32
RANDOM_BLOCK_BYTES = 64


def _seed_arg(seed):
    """the 32 seed bytes as a ctypes buffer of their own (the C entries take a host pointer); no message ever shows them"""
    if isinstance(seed, np.ndarray) and seed.dtype == np.uint8:
        seed = seed.tobytes()
    if not isinstance(seed, (bytes, bytearray)) or len(seed) != RANDOM_SEED_BYTES:
        raise ValueError("seed must be %d bytes" % RANDOM_SEED_BYTES)
    return (ctypes.c_char * RANDOM_SEED_BYTES).from_buffer_copy(bytes(seed))


def _random(name, width, seed, n, stream, first, out, like):
    for what, v in (("n", n), ("stream", stream), ("first", first)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) < 1 << 64:
            raise ValueError("%s must be an integer in [0, 2^64)" % what)
    n, stream, first = int(n), int(stream), int(first)
    if first + n > 1 << 64:
        raise ValueError("first + n exceeds 2^64")
    seed = _seed_arg(seed)
    dev = bufs.device_of(out, like)
    out = bufs.output(out, (n, width), dev)
    if n:
        _call(name, dev, seed, stream, first, n, out)
    return out.reshape(n, width)


def random_bytes(seed, n_blocks, stream=0, first=0, out=None, like=None):
    """[n_blocks, 64]: the ChaCha20 blocks first .. first + n_blocks - 1 of `stream` under the 32-byte `seed` (include/gpbc_bn254_random.h:
    RFC 8439's block function, `first + i` the 64-bit block counter, `stream` the 64-bit nonce), made on the device in one launch.
    A numpy array by default; a CUDA tensor as `out` or `like` gives a tensor, enqueued on the current stream and not synchronised.
    The seed is key material: whoever holds it can recompute the output."""
    return _random("random_bytes", RANDOM_BLOCK_BYTES, seed, n_blocks, stream, first, out, like)


def fr_random(seed, n, stream=0, first=0, out=None, like=None):
    """[n, 32] scalars: scalar i is OS2IP(block first + i of `stream`) mod r, canonical — one fr.Element.SetRandom() each, but a function
    of (seed, stream, index) alone, the same from Python, C and Go (include/gpbc_bn254_random.h).  Buffers as for random_bytes.  The seed
    is key material: whoever holds it can recompute every scalar."""
    return _random("fr_random", SCALAR_BYTES, seed, n, stream, first, out, like)


def fr_set_bytes64(x, out=None):
    """[n, 32] scalars: out[i] = OS2IP(x[64 i .. 64 i + 63]) mod r, fr.Element.SetBytes / hash.BytesToField on 64-byte strings — the
    reduction of fr_random on the caller's strings.  x: n x 64 bytes, a uint8 array, bytes or a CUDA tensor; the output is of its kind
    and must not overlap it."""
    dev = bufs.device_of(x, out)
    x, n = bufs.rows(x, RANDOM_BLOCK_BYTES, "x")
    out = bufs.output(out, (n, SCALAR_BYTES), dev)
    if n:
        if _overlaps(out, x):
            raise ValueError("out overlaps x")
        _call("fr_set_bytes64", dev, x, n, out)
    return out.reshape(n, SCALAR_BYTES)


# --------------------------------------------------------------------------------------- fixed-base tables / MSM
INDEX_NONE = 0xFFFFFFFF          # GPBC_INDEX_NONE: "no term" in an index row of FixedBase.indexed
INDEXED_MAX_TERMS = 16


def _indexed(name, handle, width, index, scalars, terms, out, ok_out):
    """The arguments of FixedBase.indexed / GTFixedBase.indexed, checked, and the call gpbc_<name>: (out [n, width], ok [n])"""
    if not bufs.is_torch(index) and not isinstance(index, np.ndarray):
        irows = [list(r) if isinstance(r, (list, tuple)) else [r] for r in index]
        terms = len(irows[0]) if irows and terms is None else terms
        if any(len(r) != terms for r in irows):
            raise ValueError("index: every row needs %s entries" % terms)
        flat = [INDEX_NONE if v is None else int(v) for r in irows for v in r]
        if any(v < 0 or v > INDEX_NONE for v in flat):
            raise ValueError("index entries are unsigned 32-bit values")
        index = np.array(flat, dtype=np.uint32)
    if not isinstance(terms, (int, np.integer)) or isinstance(terms, bool) or not 1 <= int(terms) <= INDEXED_MAX_TERMS:
        raise ValueError("terms must be in 1 .. %d (got %s)" % (INDEXED_MAX_TERMS, terms))
    terms = int(terms)
    if bufs.is_torch(index):
        if str(index.dtype) not in ("torch.int32", "torch.uint32") or not index.is_contiguous():
            raise ValueError("a device index must be a contiguous int32 / uint32 tensor")
        nidx = index.numel()
    else:
        if index.dtype != np.uint32:
            raise ValueError("index must be uint32 (got %s)" % index.dtype)
        index = np.ascontiguousarray(index).reshape(-1)
        nidx = index.size
    if not bufs.is_torch(scalars) and not isinstance(scalars, (np.ndarray, bytes, bytearray)):
        srows = [list(r) if isinstance(r, (list, tuple)) else [r] for r in scalars]
        if any(len(r) != terms for r in srows):
            raise ValueError("scalars: every output needs %d scalars" % terms)
        scalars = [v for r in srows for v in r]
    k, nscalars = bufs.rows(_fr_in(scalars), SCALAR_BYTES, "scalars")
    dev = bufs.device_of(index, k, out, ok_out)
    if nscalars % terms or nidx % terms:
        raise ValueError("scalars and index need whole rows of %d" % terms)
    n, nrows = nscalars // terms, nidx // terms
    if n and not 1 <= nrows <= n:
        raise ValueError("index needs between 1 and n = %d rows (got %d)" % (n, nrows))
    if n * terms >> 32:
        raise ValueError("n * terms must stay below 2^32")
    out = bufs.output(out, (n, width), dev)
    ok = bufs.output(ok_out, (n,), dev, "ok")
    if n:
        if not handle:
            raise ValueError("the table is closed")
        idx_bytes = index.view(np.uint8) if dev is None else None
        if _overlaps(out, idx_bytes, k) or (ok_out is not None and _overlaps(ok, idx_bytes, k, out)):
            raise ValueError("out overlaps an input")
        _call(name, dev, handle, index, nrows, terms, k, n, out, ok)
    return out, ok


class FixedBase:
    """8-bit window tables of a fixed set of bases kept in HBM (1 MB per G1 base, 2 MB per G2 base): afterwards a term of
    a sum costs 32 mixed additions and no doublings.  Serves (*G1Affine|*G2Affine).ScalarMultiplicationBase (one base: the
    generator) and the commitment loops  sum_j [c_j] srs_j  of bibe/afp25_bibe/afp25_bibe_utils.go:44-55.

        fb = FixedBase(bases, g2=False)          # bases: [nbase, 64|128] uint8 (numpy or CUDA tensor)
        out = fb.msm(scalars)                    # scalars: [n_msm, nbase] ints / [n_msm * nbase, 32] bytes -> [n_msm, 64|128]
        out = fb.mul(scalars)                    # nbase == 1: out[i] = [scalars[i]] base
    """

    def __init__(self, bases, g2=False):
        self._lib = _lib.load()
        self.g2 = bool(g2)
        self.width = G2_BYTES if g2 else G1_BYTES
        self._h = ctypes.c_void_p()
        dev = bufs.device_of(bases)
        bases, self.nbase = bufs.rows(bases, self.width, "bases")
        # Called directly, not through _call: the two forms have different shapes (one host symbol per group; the device symbol
        # takes the group as a flag and the stream before the handle), and the device form synchronises.
        if dev is None:
            _ensure_init()
            fn = self._lib.gpbc_g2_fixed_base_create if g2 else self._lib.gpbc_g1_fixed_base_create
            _lib.check(fn(bufs.address(bases), self.nbase, ctypes.byref(self._h)))
        else:
            _bind(dev)
            _lib.check(self._lib.gpbc_fixed_base_create_dev(int(self.g2), bufs.address(bases), self.nbase, _torch_stream(), ctypes.byref(self._h)))
            _current_stream().synchronize()                      # `bases` may be released by the caller after this returns

    def table_bytes(self):
        return int(self._lib.gpbc_fixed_base_table_bytes(self.nbase, int(self.g2)))

    def msm(self, scalars):
        k = scalars_to_bytes(scalars) if not (isinstance(scalars, list) and scalars and isinstance(scalars[0], (list, tuple))) \
            else scalars_to_bytes([s for row in scalars for s in row])
        dev = bufs.device_of(k)
        k, nscalars = bufs.rows(k, SCALAR_BYTES, "scalars")
        if nscalars % self.nbase:
            raise ValueError("need nbase = %d scalars per sum" % self.nbase)
        n = nscalars // self.nbase
        out = bufs.output(None, (n, self.width), dev)
        # only the device form takes a caller-side workspace; it is freed on return, hence the synchronise
        ws = () if dev is None else _workspace(None, int(self._lib.gpbc_fixed_base_msm_workspace_bytes(self._h, n)), dev)
        _call("fixed_base_msm", dev, self._h, k, n, out, *ws)
        if dev is not None:
            _current_stream().synchronize()
        return out

    def mul(self, scalars):
        if self.nbase != 1:
            raise ValueError("mul() is the single-base form; use msm()")
        return self.msm(scalars)

    def indexed(self, index, scalars, terms=None, out=None):
        """(out [n, 64|128], ok [n]): out[i] = sum_{t < terms} [scalars[i][t]] base[index[i % rows][t]] (include/gpbc_bn254_indexed.h).
        index: rows x terms entries as a uint32 array / CUDA tensor of the int32 or uint32 kind with `terms`, or a list of rows with None
        (INDEX_NONE) for "no term"; rows == n gives every output its own row, fewer rows repeat with that period.  scalars: [n][terms]
        ints or n x terms scalar rows, any value below 2^256, used as they are (so [r] B is infinity).  1 <= terms <= 16.  An index
        >= nbase other than INDEX_NONE gives an all-zero row and ok = 0.  CUDA tensors in give CUDA tensors out, enqueued on the
        current stream and not synchronised."""
        return _indexed("fixed_base_indexed", self._h, self.width, index, scalars, terms, out, None)

    def openings(self, ids, counts, coeffs=None, out=None, ok_out=None):
        """(points [n, 64|128], ok [n]): the opening proofs of n identities in k batches against this table, whose base c stands for
        [tau^c] (include/gpbc_bn254_openings.h): points[i] = [f_j(tau) / (tau - ids[i])] for identity i of batch j, f_j the product of
        (X - id) over the batch; ok[i] = 1 iff the identity is a root of f_j exactly once (gwww25_bibe.go:214-223, afp25_bibe.go:371-381),
        otherwise the row is all zero.  ids: n Python ints or scalar rows (uint8 array / CUDA tensor); counts: the k batch sizes, each at
        most min(nbase - 1, 1024), or an int B for whole batches of B; coeffs: the f_j as fr_poly_from_roots_segments(ids, counts, nbase)
        gives them (computed here when None).  CUDA tensors in give CUDA tensors out, enqueued on the current stream and not
        synchronised: the workspace is a tensor of that stream, which the allocator hands on to later work of the same stream only."""
        i, n = _flat_scalars(ids, "ids")
        if coeffs is not None:
            coeffs = _fr_in(coeffs)
        dev = bufs.device_of(i, coeffs, out, ok_out)
        seg, k = _segment_counts(counts, n, min(FR_POLY_MAX_B, self.nbase - 1), "ids")
        if coeffs is not None:
            coeffs, nc = bufs.rows(coeffs, SCALAR_BYTES, "coeffs")
            if nc != k * self.nbase:
                raise ValueError("coeffs holds %d scalars, expected %d rows of nbase = %d" % (nc, k, self.nbase))
        out = bufs.output(out, (n, self.width), dev)
        ok = bufs.output(ok_out, (n,), dev, "ok")
        if not n:
            return out, ok
        if not self._h:
            raise ValueError("the table is closed")
        if _overlaps(out, i, coeffs) or (ok_out is not None and _overlaps(ok, i, coeffs, out)):
            raise ValueError("out overlaps an input")
        if coeffs is None:
            coeffs = fr_poly_from_roots_segments(i, seg[1:] - seg[:-1], self.nbase).reshape(-1)
        ws = () if dev is None else _workspace(None, int(self._lib.gpbc_fixed_base_openings_workspace_bytes(self._h, n)), dev)
        _call("fixed_base_openings", dev, self._h, coeffs, i, seg, k, out, ok, *ws)
        return out, ok

    def close(self):
        if self._h:
            self._lib.gpbc_fixed_base_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GTFixedBase:
    """8-bit window tables of a fixed set of GT elements kept in HBM (include/gpbc_bn254_gtfixed.h, 4 MiB per base): afterwards a power
    costs 32 Fp12 products and no squarings, where gt_exp on a replicated base does 252 squarings and 77 products.  Serves the blinding
    factor of every Encrypt — e(g1, g2)^s (ibe/bb04_sibe/bb04_sibe.go:195-200), e(g1^alpha, g2)^t (ibe/bb04_ibe/bb04_ibe.go:181-189,
    ibe/waters05_ibe/waters05_ibe.go:214), and Gentry06's v, w and y.  A base is any Fp12 element, as for gt_exp.

        fb = GTFixedBase(bases)                  # bases: [nbase, 384] uint8 (numpy or CUDA tensor)
        out = fb.pow(scalars, base=0)            # out[i] = bases[base] ^ scalars[i]                              -> [n, 384]
        out, ok = fb.indexed(index, scalars)     # out[i] = prod_t bases[index[i % rows][t]] ^ scalars[i][t]      -> [n, 384], [n]

    A table from a CUDA tensor is built on the current torch stream, and the constructor waits for that build."""

    def __init__(self, bases):
        self._lib = _lib.load()
        self._h, self._rows = ctypes.c_void_p(), {}
        dev = bufs.device_of(bases)
        bases, self.nbase = bufs.rows(bases, GT_BYTES, "bases")
        if not self.nbase:
            raise ValueError("a table needs at least one base")
        # called directly, as FixedBase does: the device form takes the stream before the handle
        if dev is None:
            _ensure_init()
            _lib.check(self._lib.gpbc_gt_fixed_base_create(bufs.address(bases), self.nbase, ctypes.byref(self._h)))
        else:
            _bind(dev)
            _lib.check(self._lib.gpbc_gt_fixed_base_create_dev(bufs.address(bases), self.nbase, _torch_stream(), ctypes.byref(self._h)))
            _current_stream().synchronize()                      # `bases` may be released by the caller after this returns

    def table_bytes(self):
        return int(self._lib.gpbc_gt_fixed_base_table_bytes(self.nbase))

    def pow(self, scalars, base=0, out=None):
        """[n, 384]: out[i] = bases[base] ^ scalars[i], gnark's GT.Exp with the scalar as the integer it is (below 2^256).  scalars: n
        ints or scalar rows, host or CUDA; the output is of their kind (the one index row is made here and put where they are)."""
        if not isinstance(base, (int, np.integer)) or isinstance(base, bool) or not 0 <= int(base) < self.nbase:
            raise ValueError("base must be in 0 .. %d (got %s)" % (self.nbase - 1, base))
        key = (int(base), scalars.device if bufs.is_torch(scalars) else None)
        row = self._rows.get(key)
        if row is None:                                              # a device row travels once per table, not once per call
            row = np.array([int(base)], dtype=np.uint32)
            row = self._rows[key] = bufs.put(row.view(np.int32), scalars) if bufs.is_torch(scalars) else row
        return self.indexed(row, scalars, terms=1, out=out)[0]

    def indexed(self, index, scalars, terms=None, out=None, ok_out=None):
        """(out [n, 384], ok [n]): out[i] = prod_{t < terms} bases[index[i % rows][t]] ^ scalars[i][t].  The arguments are those of
        FixedBase.indexed: index as a uint32 array / CUDA tensor of the int32 or uint32 kind with `terms`, or a list of rows with None
        (INDEX_NONE) for "no term" — a row of nothing else gives one; rows == n gives every output its own row, fewer rows repeat with that
        period.  scalars: [n][terms] ints or n x terms scalar rows, any value below 2^256, used as they are.  1 <= terms <= 16.  An index
        >= nbase other than INDEX_NONE gives an all-zero row and ok = 0.  CUDA tensors in give CUDA tensors out, enqueued on the
        current stream and not synchronised."""
        return _indexed("gt_fixed_base_indexed", self._h, GT_BYTES, index, scalars, terms, out, ok_out)

    def close(self):
        if self._h:
            self._lib.gpbc_gt_fixed_base_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------------------------------- bit-selected sums over a fixed set
SUBSET_MAX_BITS = 16384


def _subset_points(bases, offset, width):
    """(kind, bases, nbits, offset) of a table's points, checked: whole points, 1 .. SUBSET_MAX_BITS of them, an offset of exactly one"""
    dev = bufs.device_of(bases, offset)
    bases, nbits = bufs.rows(bases, width, "bases")
    if not 1 <= nbits <= SUBSET_MAX_BITS:
        raise ValueError("a subset table takes 1 .. %d bases (got %d)" % (SUBSET_MAX_BITS, nbits))
    if offset is not None:
        offset, k = bufs.rows(offset, width, "offset")
        if k != 1:
            raise ValueError("offset must be one point of %d bytes" % width)
    return dev, bases, nbits, offset


def _subset_masks(masks, nbits):
    """(kind, flat masks, n): masks as n rows of W = ceil(nbits / 8) bytes.  [n, W] uint8 (array or CUDA tensor) goes as it is; a host
    [n, nbits] array of 0 / 1 is packed with numpy.packbits (most significant bit first: the reference's Id[] order).  For nbits = 1
    both shapes are [n, 1]: the row is then the packed byte (0x80 selects the base)."""
    W = (nbits + 7) // 8
    dev = bufs.device_of(masks)
    if dev is None:
        try:
            masks = np.asarray(masks)
        except ValueError:
            raise ValueError("masks must be a rectangular [n, %d] byte array or [n, %d] 0 / 1 array" % (W, nbits)) from None
        if masks.dtype == object:
            raise ValueError("masks must be a rectangular [n, %d] byte array or [n, %d] 0 / 1 array" % (W, nbits))
    if masks.ndim != 2 or masks.shape[1] not in (W, nbits):
        raise ValueError("masks must be [n, %d] bytes or [n, %d] bits (got shape %s)" % (W, nbits, tuple(masks.shape)))
    if masks.shape[1] != W:
        if dev is not None:
            raise ValueError("device masks must be packed: [n, %d] uint8" % W)
        if ((masks != 0) & (masks != 1)).any():
            raise ValueError("a bit array may hold only 0 and 1")
        masks = np.packbits(masks.astype(np.uint8), axis=1)
    elif dev is None and (masks.dtype.kind not in "ui" or masks.size and (masks.min() < 0 or masks.max() > 255)):
        raise ValueError("mask bytes must be integers in 0 .. 255")
    flat, n = bufs.rows(masks, W, "masks")
    return dev, flat, n


class SubsetTable:
    """Subset-sum tables of a fixed set of points over 8-bit windows of a BIT STRING, kept in HBM (include/gpbc_bn254_subset.h):
    afterwards  offset + sum_{i : bit i} bases[i]  costs one mixed addition per mask byte and no doublings, from the mask alone.
    Serves the Waters hash U' + sum_{Id[i]=1} U_i (ibe/waters05_ibe/waters05_ibe.go:172-179, 226-233) and sums of members' keys under
    a participation bitmap.  256 rows of 128 B (G1) / 256 B (G2) per 8 bases: 2 MiB for Waters05's 256 G2 points.

        t = SubsetTable(bases, offset=None, g2=False)   # bases: [nbits, 64|128] uint8, offset: one point or None (numpy or CUDA tensors)
        out = t.sum(masks)                              # masks: [n, ceil(nbits / 8)] uint8 (bit 7 - t of byte w selects bases[8 w + t],
                                                        # numpy.packbits' order) or a host [n, nbits] 0 / 1 array -> [n, 64|128]

    Device points are read by a build enqueued on the current torch stream (the table keeps them alive); host masks give a host
    array, CUDA masks a CUDA tensor enqueued on the current stream and not synchronised.  Argument errors are ValueError before any C call."""

    def __init__(self, bases, offset=None, g2=False):
        self.g2 = bool(g2)
        self.width = G2_BYTES if g2 else G1_BYTES
        self._h = ctypes.c_void_p()
        dev, bases, self.nbits, offset = _subset_points(bases, offset, self.width)
        self.W = (self.nbits + 7) // 8
        self._lib = _lib.load()
        off = None if offset is None else bufs.address(offset)
        # called directly, as FixedBase does: one host symbol per group, the device symbol takes the group as a flag and the stream before the handle
        if dev is None:
            _ensure_init()
            fn = self._lib.gpbc_g2_subset_table_create if g2 else self._lib.gpbc_g1_subset_table_create
            _lib.check(fn(bufs.address(bases), self.nbits, off, ctypes.byref(self._h)))
        else:
            _bind(dev)
            _lib.check(self._lib.gpbc_subset_table_create_dev(int(self.g2), bufs.address(bases), self.nbits, off, _torch_stream(), ctypes.byref(self._h)))
            self._points = (bases, offset)                       # the build may still be reading them
            self._build_stream = _current_stream()               # ... and is ordered on this stream alone (see _after_build)

    _points = _build_stream = None

    def _after_build(self, dev):
        """A table built from device points is ordered on the stream it was built on.  The host form runs on a stream of the library's
        own, so it waits for the build once; a device sum on another torch stream is put behind the build."""
        if self._build_stream is None:
            return
        if dev is None:
            self._build_stream.synchronize()
            self._points = self._build_stream = None
        elif _current_stream() != self._build_stream:
            _current_stream().wait_stream(self._build_stream)

    def table_bytes(self):
        return int(self._lib.gpbc_subset_table_bytes(self.nbits, int(self.g2)))

    def workspace_bytes(self, n):
        return int(self._lib.gpbc_subset_sum_workspace_bytes(self._h, n))

    def sum(self, masks, out=None, workspace=None):
        dev, masks, n = _subset_masks(masks, self.nbits)
        bufs.device_of(masks, out)
        out = bufs.output(out, (n, self.width), dev)
        if not self._h:
            raise ValueError("the table is closed")
        if dev is None:
            if workspace is not None:
                raise ValueError("only the device form takes a workspace")
            self._after_build(None)
            _call("subset_sum", None, self._h, masks, n, out)
            return out
        _bind(dev)
        self._after_build(dev)
        need = self.workspace_bytes(n)
        ws = (None, 0) if not need and workspace is None else _workspace(workspace, need, dev)
        _call("subset_sum", dev, self._h, masks, n, out, *ws)
        return out

    def close(self):
        if self._h:
            self._lib.gpbc_subset_table_destroy(self._h)
            self._h = ctypes.c_void_p()
            self._points = self._build_stream = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _subset_sum(g2, bases, masks, offset, out):
    width = G2_BYTES if g2 else G1_BYTES
    pdev, bases, nbits, offset = _subset_points(bases, offset, width)
    dev, flat, n = _subset_masks(masks, nbits)
    if (pdev is None) != (dev is None) or (dev is not None and dev != pdev):
        raise ValueError("the buffers of one call must all be CUDA tensors on one device or all host buffers")
    bufs.device_of(flat, out)
    out = bufs.output(out, (n, width), dev)
    table = SubsetTable(bases, offset, g2=g2)
    try:
        return table.sum(flat.reshape(n, -1), out=out)
    finally:
        table.close()                                            # drains the device: the result is there on return


def g1_subset_sum(bases, masks, offset=None, out=None):
    """out[m] = offset + sum_{i : bit i of masks[m]} bases[i] in G1 with a table built for this one call (SubsetTable keeps it)."""
    return _subset_sum(False, bases, masks, offset, out)


def g2_subset_sum(bases, masks, offset=None, out=None):
    return _subset_sum(True, bases, masks, offset, out)
