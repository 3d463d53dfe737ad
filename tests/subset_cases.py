"""Case list of the bit-selected sums over a fixed set (csrc/subset29.hip.hpp), shared by the CPU harness test (test_subset_sum.py)
and the GPU test (test_subset_sum_gpu.py): tables (a base set, an offset, a size) with their masks, and the expected bytes from the
oracle — oracle_lib.g1_sum / g2_sum over [O] + the bases a mask selects, numpy.unpackbits giving the selection (the reference's Id[]
order: most significant bit of every byte first, positions >= nbits of the last byte selecting nothing).

Base sets (every point a multiple of the generator made by the oracle's scalar multiplication; a negative is the multiple by r - k):
    rand    distinct multiples                         same    every B_i = P
    pairs   B_{2j+1} = -B_{2j}                         mirror  B_{8+t} = -B_t for t < 8 (the rest distinct)
    holes   every third base all zero (infinity)
Offsets: none, a point, infinity (all zero), -B_0.  Sizes: 1, 7, 8, 9, 255, 256, 257 and 2048 (the chunked route: 256 windows cut into
8 chunks of 32 for any call below 131072 items).

Every table gets the masks of common_masks (all zero, all ones with and without the padding bits of the last byte, 0x80, 0xC0,
0x80 0x80, 0x80 0x80 .. 0x80, three SHA-256 digests); `rand` without an offset and with one also gets one bit at every position.  What
the named masks reach:
    0x80 0x80 on `same`        the accumulator P meets the entry P: jac_add_mixed doubles                    -> 2P
    0x80 0x80 on `mirror`      the accumulator B_0 meets -B_0: infinity; "then 0x80" carries on from infinity  -> B_16
    0xC0 on `pairs`            the entry B_0 + B_1 is infinity (flagged); with an offset the entry is O        -> infinity / O
    0x80 with offset -B_0      entry (0, 0x80) = O + B_0 is infinity                                           -> infinity
test_subset_sum.py asserts those from the expected bytes alone."""
import hashlib

import numpy as np

import bn254_py as o

R = o.R
BYTES = {False: 64, True: 128}
SIZES = [1, 7, 8, 9, 255, 256, 257, 2048]
SETS = ["rand", "same", "pairs", "mirror", "holes"]
OFFSETS = ["none", "point", "inf", "-B0"]
DIGESTS = ["alice@example.com", "bob", "身份"]
MAX_BITS = 16384


def krows(ks):
    return np.frombuffer(b"".join((int(k) % R).to_bytes(32, "little") for k in ks), dtype=np.uint8).reshape(-1, 32).copy()


def gen_multiples(oracle, g2, ks):
    """[k] g for every k, [len(ks), 64 | 128]"""
    gen = np.frombuffer(o.g2_to_bytes(o.G2_GEN) if g2 else o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
    return np.asarray((oracle.g2_scalar_mul if g2 else oracle.g1_scalar_mul)(gen, krows(ks).reshape(-1), threads=8)).reshape(-1, BYTES[g2])


def base_scalars(name, nbits):
    """log_g of every base; None = the point at infinity"""
    k = [1000 + 17 * i for i in range(nbits)]
    if name == "same":
        k = [4242] * nbits
    elif name == "pairs":
        k = [k[i - 1] * (R - 1) % R if i & 1 else k[i] for i in range(nbits)]
    elif name == "mirror":
        k = [k[i - 8] * (R - 1) % R if 8 <= i < 16 else k[i] for i in range(nbits)]
    elif name == "holes":
        k = [None if i % 3 == 2 else k[i] for i in range(nbits)]
    return k


OFFSET_SCALAR = 777777


def offset_scalar(name, base_k):
    """log_g of the offset: "none" -> no offset at all, None -> the all-zero point"""
    if name == "point":
        return OFFSET_SCALAR
    if name == "-B0":
        return None if base_k[0] is None else (R - base_k[0]) % R
    return None


def digest_mask(s, W):
    d = hashlib.sha256(s.encode()).digest()
    return np.frombuffer((d * (W // 32 + 1))[:W], dtype=np.uint8)


def common_masks(nbits):
    """[(name, row of W bytes)]"""
    W = (nbits + 7) // 8
    z = lambda: np.zeros(W, dtype=np.uint8)
    pad_clear = np.packbits(np.ones(nbits, dtype=np.uint8))
    out = [("zero", z()), ("ones", np.full(W, 0xFF, dtype=np.uint8)), ("ones, padding clear", pad_clear)]
    for name, head in (("0x80", [0x80]), ("0xC0", [0xC0]), ("0x80 0x80", [0x80, 0x80]), ("0x80 0x80, then 0x80", [0x80, 0x80, 0x80])):
        if len(head) <= W:
            m = z()
            m[:len(head)] = head
            out.append((name, m))
    if nbits % 8:                                                 # the padding bits alone, and under a one-bit mask
        m = z()
        m[-1] = 0xFF >> (nbits % 8)
        out.append(("padding bits only", m))
        m = m.copy()
        m[0] |= 0x80
        out.append(("0x80 and the padding bits", m))
    out += [("sha256 %d" % i, digest_mask(s, W)) for i, s in enumerate(DIGESTS)]
    return out


def one_bit_masks(nbits):
    return np.packbits(np.eye(nbits, dtype=np.uint8), axis=1)


class Table:
    def __init__(self, label, B, O, nbits, names, masks):
        self.label, self.B, self.O, self.nbits, self.names, self.masks = label, B, O, nbits, names, masks

    def row(self, name):
        return self.names.index(name)


_TABLES, _EXPECT = {}, {}


def _points(oracle, g2, ks):
    """points for a list of logs with None = infinity; every distinct log is multiplied once"""
    distinct = sorted({k for k in ks if k is not None})
    rows = dict(zip(distinct, gen_multiples(oracle, g2, distinct))) if distinct else {}
    zero = np.zeros(BYTES[g2], dtype=np.uint8)
    return np.stack([zero if k is None else rows[k] for k in ks])


def make_table(oracle, g2, set_name, off_name, nbits, extra_masks=None, one_bits=False):
    bk = base_scalars(set_name, nbits)
    B = _points(oracle, g2, bk)
    O = None if off_name == "none" else _points(oracle, g2, [offset_scalar(off_name, bk)])[0]
    named = common_masks(nbits)
    names, masks = [n for n, _ in named], [m for _, m in named]
    if one_bits:
        ob = one_bit_masks(nbits)
        names += ["bit %d" % i for i in range(nbits)]
        masks += list(ob)
    if extra_masks is not None:
        names += ["extra %d" % i for i in range(len(extra_masks))]
        masks += list(extra_masks)
    return Table("%s/%s/%d" % (set_name, off_name, nbits), B, O, nbits, names, np.stack(masks))


def tables(oracle, g2):
    if g2 not in _TABLES:
        _TABLES[g2] = [make_table(oracle, g2, s, off, nbits, one_bits=(s == "rand" and off in ("none", "point")))
                       for nbits in SIZES for s in SETS for off in OFFSETS]
    return _TABLES[g2]


def expect(oracle, g2, t, masks=None):
    """the oracle's sum over [O] + the selected bases, one row per mask"""
    masks = t.masks if masks is None else np.asarray(masks, dtype=np.uint8).reshape(-1, (t.nbits + 7) // 8)
    add = oracle.g2_sum if g2 else oracle.g1_sum
    sel = np.unpackbits(masks, axis=1)[:, :t.nbits].astype(bool)
    out = np.zeros((len(masks), BYTES[g2]), dtype=np.uint8)
    head = [] if t.O is None else [t.O[None]]
    for m in range(len(masks)):
        pts = np.concatenate(head + [t.B[sel[m]]]) if head or sel[m].any() else None
        if pts is not None and len(pts):
            out[m] = add(pts)
    return out


def expected(oracle, g2):
    """label -> expected rows of every table of the list, computed once per session"""
    if g2 not in _EXPECT:
        _EXPECT[g2] = {t.label: expect(oracle, g2, t) for t in tables(oracle, g2)}
    return _EXPECT[g2]


def random_masks(tag, n, W):
    rng = np.random.default_rng(int.from_bytes(hashlib.sha256(tag.encode()).digest()[:4], "little"))
    return rng.integers(0, 256, size=(n, W), dtype=np.uint8)


def multiple(oracle, g2, k):
    return gen_multiples(oracle, g2, [k])[0]
