"""Case list and expectation of the XOR mask from GT bytes (csrc/mask29.hip.hpp, include/gpbc_bn254_mask.h), shared by
test_gt_xor_mask.py (CPU) and test_gt_xor_mask_gpu.py.

The expectation is pure Python: oracle/bn254_py.py's gt_to_canonical_bytes — GT.Bytes(), the twelve coefficients big-endian canonical
from C1.B2.A1 down to C0.B0.A0 — XOR the message, cut to the shorter of the two (utils/xor.go:3-16), zero beyond.  It shares nothing
with the kernel.

GT inputs (KINDS): zero, one, a pairing value, every coefficient p - 1, and an element whose first used coefficient (C1.B2.A1, bytes
0..31 of the mask) is 0 while the next is not.  Lengths (LENGTHS): 0, 1, 31, 32, 33, 63, 64, 65, 383, 384, 385, 500 — each side of every
32-byte piece boundary, of the 384-byte cut, and a tail of more than one zero piece per lane.  A ragged case of n items takes the
lengths in the order ORDER — a 1-byte message first, so that the offsets behind it are odd, and the zero-length item in the middle — and
the GT kinds in turn: 12 and 5 are coprime, so the 65-item case holds every (length, kind) pair.  The message buffer has LEAD bytes in
front of the first message and TRAIL behind the last, which no item owns; with LEAD = 15 whole pieces occur at 16-byte, at 4-byte and
at odd addresses (relative to the buffer's start), which are the kernel's three access paths.  Item counts: 1, 21, 22 (22 x 12 lanes cross a 256-lane
workgroup) and 65 (more items than a wavefront has lanes).  Row cases: width 1, 32, 33, 384, 400 — the row form launches only the
windows a row can reach, 1, 1, 2, 12 and 12 lanes per item — at ROWS = 300 rows, which cross a 256-lane workgroup at one lane per item
too.  Every case is also run in place by the GPU tests."""
import hashlib

import numpy as np

import bn254_py as o

P = o.P
LENGTHS = [0, 1, 31, 32, 33, 63, 64, 65, 383, 384, 385, 500]
ORDER = [1, 31, 32, 33, 63, 64, 0, 65, 383, 384, 385, 500]
COUNTS = [1, 21, 22, 65]
WIDTHS = [1, 32, 33, 384, 400]
ROWS = 300
LEAD, TRAIL = 15, 5
MASK_BYTES = 384


def _f12(coeffs):
    """twelve integers in memory order (C0.B0.A0 first) as the oracle's nested tuples"""
    c = [(coeffs[2 * i], coeffs[2 * i + 1]) for i in range(6)]
    return ((c[0], c[1], c[2]), (c[3], c[4], c[5]))


def _kinds():
    zero_then_not = [(7 * k + 3) * 0x0123456789ABCDEF % P for k in range(12)]
    zero_then_not[11] = 0                                        # C1.B2.A1 = 0: mask bytes 0..31 are zero, bytes 32..63 are not
    elems = [("zero", _f12([0] * 12)), ("one", o.F12_ONE), ("pairing", o.pair([o.G1_GEN], [o.G2_GEN])), ("p-1", _f12([P - 1] * 12)),
             ("first-zero", _f12(zero_then_not))]
    return [(name, np.frombuffer(o.gt_to_bytes(e), dtype=np.uint8), o.gt_to_canonical_bytes(e)) for name, e in elems]


KINDS = _kinds()                                                 # (name, the 384 in-memory bytes, GT.Bytes())
KIND_NAMES = [k[0] for k in KINDS]


def mask_of(row):
    """GT.Bytes() of one in-memory GT row, through the oracle's decoding"""
    return o.gt_to_canonical_bytes(o.gt_from_bytes(np.asarray(row, dtype=np.uint8).tobytes()))


def message(label, i, length):
    return hashlib.shake_256(("%s/%d" % (label, i)).encode()).digest(length)


def xor_cut(msg, mask):
    """(out, L): utils.Xor's slice, then zeros up to the message's length"""
    L = min(len(msg), len(mask))
    return bytes(a ^ b for a, b in zip(msg[:L], mask[:L])) + bytes(len(msg) - L), L


def _case(label, kinds, msgs, lead, trail, width):
    gt = np.stack([KINDS[k][1] for k in kinds]) if kinds else np.zeros((0, MASK_BYTES), dtype=np.uint8)
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    off[0] = lead
    off[1:] = lead + np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    canary = lambda k, salt: bytes((0xC3 + 29 * j + salt) % 256 or 1 for j in range(k))
    data = np.frombuffer(canary(lead, 0) + b"".join(msgs) + canary(trail, 7), dtype=np.uint8).copy()
    outs = [xor_cut(m, KINDS[k][2]) for m, k in zip(msgs, kinds)]
    want = np.frombuffer(canary(lead, 0) + b"".join(x for x, _ in outs) + canary(trail, 7), dtype=np.uint8).copy()
    return dict(label=label, n=len(msgs), kinds=list(kinds), gt=gt, msgs=list(msgs), data=data, off=off, width=width, want=want,
                want_len=np.array([L for _, L in outs], dtype=np.uint32))


def ragged_case(n):
    label = "ragged-%d" % n
    lengths = [ORDER[i % len(ORDER)] for i in range(n)]
    return _case(label, [i % len(KINDS) for i in range(n)], [message(label, i, L) for i, L in enumerate(lengths)], LEAD, TRAIL, None)


def row_case(width, n=ROWS):
    label = "rows-%d" % width
    return _case(label, [(i + 2) % len(KINDS) for i in range(n)], [message(label, i, width) for i in range(n)], 0, 0, width)


_CASES = None


def cases():
    """the whole list, made once and never changed by a test (tests copy what they hand to an entry)"""
    global _CASES
    if _CASES is None:
        _CASES = [ragged_case(n) for n in COUNTS] + [row_case(w) for w in WIDTHS]
    return _CASES


def case_ids():
    return ["ragged-%d" % n for n in COUNTS] + ["rows-%d" % w for w in WIDTHS]


def rows_of(case):
    """the row form of a row case: messages [n, width], expectation [n, width]"""
    return case["data"].reshape(case["n"], case["width"]), case["want"].reshape(case["n"], case["width"])
