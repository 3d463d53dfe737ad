"""Case lists of the transcript hash H(u, v, w) and of the plain SHA-256 (csrc/transcript29.hip.hpp), shared by the CPU harness test
(test_transcript_hash.py) and the GPU test (test_transcript_hash_gpu.py).  Expected values come from hashlib over the oracle's own
encoders (bn254_py.g1_marshal(compressed=True), gt_marshal): nothing of the code under test takes part in them.

Transcript items: u in {infinity, the generator, a point and its negative (both Y flags), a point whose X has a leading zero byte (found
by a seeded walk over [k] g1, if one turns up within 2^12 steps)} x (v, w) in {zero, one, a pairing value, 12 x (p - 1)}^2, then 32
seeded items of random multiples of g1 and GT structs of random coefficients (H makes no membership test, so any twelve field elements
are a GT input).  SHA-256 messages: every length at which the padding changes shape — 0, 1, 55 | 56 (the length field moves to a second
block), 63, 64, 65, 119 | 120, 127, 128 — and 1000 bytes, plus the two published vectors."""
import hashlib

import numpy as np

import bn254_py as o

R, P = o.R, o.P
SHA_LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 1000]
# FIPS 180-4 / NIST CSRC "SHA-256 example" vectors: the one-block message "abc" and the empty string
KNOWN = [(b"abc", "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"),
         (b"", "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855")]
_CACHE = {}


def _rand(tag, i, mod):
    return int.from_bytes(hashlib.sha512(("transcript-%s-%d" % (tag, i)).encode()).digest(), "big") % mod


def leading_zero_point():
    """(k, [k] g1) with X < 2^248 — the first byte of G1Affine.Bytes() is then the bare flag — or None after 2^12 steps"""
    k0 = _rand("walk", 0, R)
    pt = o.g1_mul(o.G1_GEN, k0)
    for step in range(1 << 12):
        if pt[0] < (1 << 248):
            return k0 + step, pt
        pt = o.g1_add(pt, o.G1_GEN)
    return None


def gt_edges(oracle):
    """name -> GT struct as the oracle's tuple"""
    if "gt" not in _CACHE:
        g1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
        g2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
        zero = (((0, 0),) * 3,) * 2
        _CACHE["gt"] = {"zero": zero, "one": (((1, 0), (0, 0), (0, 0)), ((0, 0),) * 3),
                        "pair": o.gt_from_bytes(np.asarray(oracle.pair_batch(g1, g2)).tobytes()), "p-1": (((P - 1, P - 1),) * 3,) * 2}
    return _CACHE["gt"]


def transcript_items(oracle):
    """[(name, u point or None, v tuple, w tuple)]"""
    if "items" not in _CACHE:
        five = o.g1_mul(o.G1_GEN, 5)
        us = [("inf", None), ("gen", o.G1_GEN), ("5g", five), ("-5g", o.g1_neg(five))]
        lz = leading_zero_point()
        if lz is not None:
            us.append(("x<2^248", lz[1]))
        gts = gt_edges(oracle)
        items = [("%s/%s/%s" % (un, vn, wn), u, v, w) for un, u in us for vn, v in gts.items() for wn, w in gts.items()]
        ks = np.frombuffer(b"".join(_rand("k", i, R).to_bytes(32, "little") for i in range(32)), dtype=np.uint8)
        g1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
        pts = np.asarray(oracle.g1_scalar_mul(g1, ks, threads=8)).reshape(32, 64)
        coeff = lambda i, t: tuple(tuple((_rand("c%d" % t, 12 * i + 2 * (3 * h + c), P), _rand("c%d" % t, 12 * i + 2 * (3 * h + c) + 1, P)) for c in range(3)) for h in range(2))
        items += [("random %d" % i, o.g1_from_bytes(pts[i].tobytes()), coeff(i, 0), coeff(i, 1)) for i in range(32)]
        _CACHE["items"] = items
    return _CACHE["items"]


def transcript_arrays(oracle):
    """(names, u [n, 64], v [n, 384], w [n, 384], expected [n, 32]) — gnark in-memory structs in, scalar-format rows out"""
    if "arrays" not in _CACHE:
        items = transcript_items(oracle)
        col = lambda parts: np.frombuffer(b"".join(parts), dtype=np.uint8).reshape(len(items), -1).copy()
        want = []
        for _, u, v, w in items:
            stream = o.g1_marshal(u, compressed=True) + o.gt_marshal(v) + o.gt_marshal(w)
            assert len(stream) == 800
            want.append((int.from_bytes(hashlib.sha256(stream).digest(), "big") % R).to_bytes(32, "little"))
        _CACHE["arrays"] = ([it[0] for it in items], col([o.g1_to_bytes(it[1]) for it in items]), col([o.gt_to_bytes(it[2]) for it in items]),
                            col([o.gt_to_bytes(it[3]) for it in items]), col(want))
    return _CACHE["arrays"]


def sha_messages():
    """the messages of SHA_LENGTHS (seeded bytes), then the two published ones"""
    msgs = [hashlib.shake_128(b"transcript-msg-%d" % n).digest(n) for n in SHA_LENGTHS]
    return msgs + [m for m, _ in KNOWN]


def sha_expected(msgs, to_fr):
    rows = [hashlib.sha256(m).digest() for m in msgs]
    if to_fr:
        rows = [(int.from_bytes(d, "big") % R).to_bytes(32, "little") for d in rows]
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(msgs), 32).copy()


def flat_messages(msgs):
    """(buffer, uint64 offsets) of a message list"""
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    data = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy() if int(off[-1]) else np.zeros(1, dtype=np.uint8)
    return data, off


def rotate(a, n, shift=0):
    """n rows of `a`, cyclically from row `shift` on"""
    return np.ascontiguousarray(a[(np.arange(n) + shift) % len(a)])
