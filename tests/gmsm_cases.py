"""Case lists of the segmented G1 / G2 multi-scalar multiplication, shared by the CPU harness test (test_multi_scalar_mul.py) and the
GPU tests (test_multi_scalar_mul_gpu.py): bases, scalars, segment tables, and the expected bytes from the oracle (g*_scalar_mul per
term, the terms of a segment added up by the oracle's g*_sum).

The plan the cases aim at (csrc/segred29.hip.hpp with the shape of csrc/gmsm29.hip.hpp): a call of n terms in n_seg segments cuts every segment into
J = max(1, min(n // n_seg // G, ceil(131072 / n_seg))) pieces (plain sums: // 8), G = GMSM_GROUP read from the harness
(hc_gmsm_group), a lane takes the terms of its piece G at a time, and the J piece values of every segment are folded by the plain-sum
form of the same plan.  For one segment of L terms J = L // G, so J steps at every multiple of G; the lists hold the first steps
(1 -> 2 at 2G, 2 -> 3 at 3G) and the lengths at which a further fold level appears — 16 pieces need a second level (16G terms;
plain sums 128 points), 128 pieces a third (128G; 1024), 1024 pieces a fourth (8192 points) — each one below, at, and one above.
With scalars the list stops at the third level: the fourth would appear at 1024G terms, 12 288 terms in three calls and as many again
in each combined call, minutes on the host harness, and it would run no other code than the plain sum of 8192 points does — every
fold level IS the plain-sum kernel on uniform segments, writing the two piece-value blocks alternately, and four levels of that are
in the plain list.  Every length is a call of one segment, and all of them are one call, forwards and reversed, with an empty segment
at both ends.

Run as a script it sends the cases and the ragged calls through the host-pointer entry in a process of its own bound to the device
list given on the command line (a device may be listed twice, so one GPU still crosses the shard split, which cuts by whole segments)."""
import os
import sys

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle")]

import numpy as np  # noqa: E402

import bn254_py as o  # noqa: E402
import bounds_harness  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = o.R
BYTES = {False: 64, True: 128}
SUM_MIN, FILL = 8, 131072


def harness():
    """tools/libgpbc_bounds.so (the device arithmetic as a host build with -DGPBC_BOUNDS), through the one loader"""
    return bounds_harness.load()


def group(g2):
    return int(harness().hc_gmsm_group(int(g2)))


def pieces(n, n_seg, has_k, g2=False):
    """segred_pieces (csrc/segred29.hip.hpp) with GMSM_SHAPE, restated"""
    return max(1, min(n // n_seg // (group(g2) if has_k else SUM_MIN), -(-FILL // n_seg)))


def lengths_with_scalars(g2):
    G = group(g2)
    base = [0, 1, 2, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 3 * G - 1, 3 * G, 3 * G + 1]
    return sorted(set(L for L in base + [16 * G - 1, 16 * G, 16 * G + 1, 128 * G - 1, 128 * G, 128 * G + 1] if L >= 0))


def lengths_plain(g2):
    return sorted(set(lengths_with_scalars(g2) + [15, 16, 17, 23, 24, 25, 127, 128, 129, 1023, 1024, 1025, 8191, 8192, 8193]))


def krows(ks):
    return np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in ks), dtype=np.uint8).reshape(-1, 32).copy()


def hash_tag(tag):
    import hashlib
    return int.from_bytes(hashlib.sha256(tag.encode()).digest()[:4], "little")


def rand_scalars(tag, n):
    rng = np.random.default_rng(hash_tag(tag))
    return [int.from_bytes(rng.bytes(32), "little") for _ in range(n)]


def _cube_roots():
    g = 2
    while pow(g, (R - 1) // 3, R) == 1:
        g += 1
    w = pow(g, (R - 1) // 3, R)
    return [w, w * w % R]


MU = 6 * o.U * o.U % R                      # psi acts as [mu] on G2
EDGE_SCALARS = [0, 1, 2, 3, R - 1, R, R + 1, 1 << 255, (1 << 256) - 1]


def digit_scalars(g2):
    """one non-zero digit per window of a split half: d 4^w and (d 4^w) lambda for the two-bit windows of the GLV halves (both cube
    roots of unity: one of them is the kernel's lambda, the other -1 - lambda puts the digit into both halves); 2^w mu^i for the bits
    of the four GLS quarters"""
    if not g2:
        return [((w % 3) + 1) << (2 * w) for w in range(63)] + [(((w % 3) + 1) << (2 * w)) * lam % R for lam in _cube_roots() for w in range(63)]
    return [(1 << w) * pow(MU, i, R) % R for i in range(4) for w in range(64)]


_POOL = {}


def pool(g2):
    """12 points [a_i] G with their negatives and doubles, and the point at infinity: dict of [*, 64 | 128] uint8 rows"""
    if g2 not in _POOL:
        mul, gen, enc, neg = (o.g2_mul, o.G2_GEN, o.g2_to_bytes, o.g2_neg) if g2 else (o.g1_mul, o.G1_GEN, o.g1_to_bytes, o.g1_neg)
        pts = [mul(gen, 1000 + 17 * i) for i in range(12)]
        rows = lambda ps: np.frombuffer(b"".join(enc(p) for p in ps), dtype=np.uint8).reshape(-1, BYTES[g2]).copy()
        _POOL[g2] = {"pt": rows(pts), "neg": rows([neg(p) for p in pts]), "dbl": rows([mul(gen, 2 * (1000 + 17 * i)) for i in range(12)]),
                     "inf": np.zeros((1, BYTES[g2]), dtype=np.uint8)}
    return _POOL[g2]


def take(rows, n, start=0):
    return np.stack([rows[(start + i) % len(rows)] for i in range(n)]) if n else np.zeros((0, rows.shape[1]), dtype=np.uint8)


def offsets(lengths):
    return [0] + [int(v) for v in np.cumsum(lengths)]


_CASES = {}


def cases(g2):
    """(label, bases [n, 64 | 128], k (list of n or of m integers, or None), seg_off (list), shared)"""
    if g2 in _CASES:
        return _CASES[g2]
    p = pool(g2)
    pt, neg, dbl, inf = p["pt"], p["neg"], p["dbl"], p["inf"]
    G = group(g2)
    tag = "g2" if g2 else "g1"
    out = []
    # every length as a call of its own (one segment) and all of them in one call, random scalars
    LS = lengths_with_scalars(g2)
    for L in LS:
        out.append(("one segment of %d" % L, take(pt, L, L), rand_scalars("%s-len%d" % (tag, L), L), [0, L], False))
    # ... every one of them in one call, forwards and reversed, with empty segments at both ends (J = 22 for G = 4: several
    # segments with two fold levels, both piece-value blocks in use); and the lengths up to 16G + 1 alone (J = 4, one fold)
    n = sum(LS)
    out.append(("all lengths in one call", take(pt, n), rand_scalars(tag + "-all", n), offsets([0] + LS + [0]), False))
    out.append(("all lengths, reversed", take(pt, n, 3), rand_scalars(tag + "-rev", n), offsets([0] + LS[::-1] + [0]), False))
    short = [L for L in LS if L <= 16 * G + 1]
    n = sum(short)
    out.append(("the lengths up to 16G + 1 in one call", take(pt, n), rand_scalars(tag + "-short", n), offsets([0] + short + [0]), False))
    # G and G + 1 terms side by side in one wavefront: lanes that leave the group loop before their neighbours (the shapes on which
    # the first build of the G2 kernel was wrong on the device)
    for name, ls in (("G, G + 1", [G, G + 1]), ("G + 1, G", [G + 1, G]), ("G, 2G", [G, 2 * G]), ("G, G, G + 1", [G, G, G + 1])):
        out.append(("segments of " + name, take(pt, sum(ls), 2), rand_scalars(tag + "-side" + name, sum(ls)), offsets(ls), False))
    # the edge scalars and one digit per window position: each alone (one-term segments), then as the terms of segments of 5
    E = EDGE_SCALARS + digit_scalars(g2)
    E = E + [7] * (-len(E) % 5)
    out.append(("edge scalars, one per segment", take(pt, len(E)), E, list(range(len(E) + 1)), False))
    out.append(("edge scalars, segments of 5", take(pt, len(E), 5), E, list(range(0, len(E) + 1, 5)), False))
    out.append(("all scalars zero", take(pt, 2 * G + 1), [0, R] * G + [0], [0, G, 2 * G + 1], False))
    # points
    out.append(("infinity alone", inf, [5], [0, 1], False))
    out.append(("infinity first, last, and for a whole segment", np.concatenate([inf, pt[:2], pt[2:4], inf, inf, inf, inf]), rand_scalars(tag + "-inf", 9), [0, 3, 6, 9], False))
    out.append(("the same base through a segment", take(pt[3:4], 2 * G + 1), rand_scalars(tag + "-same", 2 * G + 1), [0, 2 * G + 1], False))
    # cancellations and doublings inside the joint loop, at the start of a group and straddling a group boundary (terms G - 1 and G)
    s = rand_scalars(tag + "-eq", 1)[0]
    quad = [("P + P", [pt[0], pt[0]], [1, 1]), ("P - P by the scalar", [pt[0], pt[0]], [1, R - 1]), ("P + (-P), equal scalars", [pt[0], neg[0]], [s, s]),
            ("2 P - 2P", [pt[0], dbl[0]], [2, R - 1])]
    for label, b, k in quad:
        out.append((label, np.stack(b), k, [0, 2], False))
        if G > 1:
            lead = G - 1
            out.append((label + ", across a group boundary", np.concatenate([take(pt, lead, 5), np.stack(b)]), [0] * lead + k, [0, lead + 2], False))
            out.append((label + ", across a group boundary, other terms around", np.concatenate([take(pt, lead, 5), np.stack(b), pt[7:8]]),
                        rand_scalars(tag + label, lead) + k + [11], [0, lead + 3], False))
    out.append(("infinity mid-segment, then more terms", np.stack([pt[0], neg[0], pt[1], pt[2], inf[0], pt[3]]), [9, 9, 5, 6, 7, 8], [0, 6], False))
    out.append(("the sum passes through infinity between groups", np.concatenate([take(pt, G), take(neg, G), pt[5:6]]), list(range(3, 3 + G)) * 2 + [R - 2], [0, 2 * G + 1], False))
    # the shared scalar list (nk = m for segments of m) and the plain sum (k = None)
    for m, segs in ((1, 3), (G, 3), (G + 1, 2), (16, 2)):
        out.append(("shared list of %d for %d segments" % (m, segs), take(pt, m * segs, m), rand_scalars("%s-sh%d" % (tag, m), m), list(range(0, m * segs + 1, m)), True))
    out.append(("shared edge scalars", take(pt, 2 * len(EDGE_SCALARS), 1), EDGE_SCALARS, [0, len(EDGE_SCALARS), 2 * len(EDGE_SCALARS)], True))
    mix = np.concatenate([pt, neg[:3], dbl[:3], inf])
    for L in lengths_plain(g2):
        out.append(("sum of %d" % L, take(mix, L, L), None, [0, L], False))
    LP = lengths_plain(g2)
    out.append(("sums, all lengths", take(mix, sum(LP)), None, offsets([0] + LP + [0]), False))
    out.append(("sums, all lengths, reversed", take(mix, sum(LP), 7), None, offsets([0] + LP[::-1] + [0]), False))
    out.append(("P + (-P), P + P, infinity entries", np.stack([pt[0], neg[0], pt[1], pt[1], inf[0], pt[2], inf[0], inf[0], inf[0]]), None, [0, 2, 4, 7, 9], False))
    _CASES[g2] = out
    return out


def expect(oracle, g2, x, k, seg, shared, threads=1):
    """oracle scalar multiplication per term, oracle sum per segment"""
    n_seg, w = len(seg) - 1, BYTES[g2]
    x = np.ascontiguousarray(x).reshape(-1, w)
    if k is None or not len(x):
        e = x
    else:
        ks = list(k) * n_seg if shared else k
        e = (oracle.g2_scalar_mul if g2 else oracle.g1_scalar_mul)(x, krows(ks), threads=threads)
    out = np.zeros((n_seg, w), dtype=np.uint8)
    for s in range(n_seg):
        if seg[s + 1] > seg[s]:
            out[s] = (oracle.g2_sum if g2 else oracle.g1_sum)(e[seg[s]:seg[s + 1]])
    return out


_EXPECT = {}


def expected(oracle, g2):
    """label -> expected rows of every case, computed once per session"""
    if g2 not in _EXPECT:
        _EXPECT[g2] = {label: expect(oracle, g2, x, k, seg, shared) for label, x, k, seg, shared in cases(g2)}
    return _EXPECT[g2]


def ragged_case(g2, n_seg, tag):
    """n_seg segments of lengths 0 .. 5 in a fixed irregular order over pool points with random scalars: (x, k, seg)"""
    p = pool(g2)
    lengths = [(7 * i + i // 7) % 6 for i in range(n_seg)]
    seg = offsets(lengths)
    n = seg[-1]
    rows = np.concatenate([p["pt"], p["neg"][:2], p["inf"]])
    return rows[np.arange(n) % len(rows)], rand_scalars(tag, n), seg


def run_engine_cases(eng, oracle, g2, put=None, table_on_device=False):
    """every case through eng.g*_multi_scalar_mul (k = None: also eng.g*_sum_segments): numpy arrays, or with put = a host-to-device
    function CUDA tensors, the segment table on the host or on the device.  Returns the list of failures."""
    bad = []
    want_all = expected(oracle, g2)
    msm = eng.g2_multi_scalar_mul if g2 else eng.g1_multi_scalar_mul
    plain = eng.g2_sum_segments if g2 else eng.g1_sum_segments
    host = lambda a: np.asarray(a if put is None else a.cpu().numpy()).reshape(-1, BYTES[g2])
    for label, x, k, seg, shared in cases(g2):
        want = want_all[label]
        xs = np.ascontiguousarray(x).reshape(-1)
        kk = None if k is None else krows(k).reshape(-1)
        if put is None:
            got = msm(xs, kk, seg)
            alt = plain(xs, seg) if k is None else got
        else:
            table = put(np.array(seg, dtype=np.int64)) if table_on_device else seg
            got = msm(put(xs), None if kk is None else put(kk), table)
            alt = plain(put(xs), table) if k is None else got
        if not (host(got) == want).all() or not (host(alt) == want).all():
            bad.append(label)
    return bad


def shard_run(eng, oracle):
    """host-pointer calls large enough for the shard split (whole segments per shard, tables rebased): ragged segments with one
    scalar per term, equal segments with a shared list, plain sums; plus the case lists on the smaller routes"""
    bad = []
    for g2 in (False, True):
        tag = "g2 " if g2 else "g1 "
        msm = eng.g2_multi_scalar_mul if g2 else eng.g1_multi_scalar_mul
        plain = eng.g2_sum_segments if g2 else eng.g1_sum_segments
        bad += [tag + b for b in run_engine_cases(eng, oracle, g2)]
        x, k, seg = ragged_case(g2, 6000, tag + "shard-ragged")
        if not (msm(x.reshape(-1), krows(k).reshape(-1), seg) == expect(oracle, g2, x, k, seg, False, threads=16)).all():
            bad.append(tag + "shard ragged")
        if not (plain(x.reshape(-1), seg) == expect(oracle, g2, x, None, seg, False)).all():
            bad.append(tag + "shard sums")
        m, segs = 3, 3000
        xs, ks, table = x[:m * segs], rand_scalars(tag + "shard-shared", m), list(range(0, m * segs + 1, m))
        if not (msm(xs.reshape(-1), krows(ks).reshape(-1), table) == expect(oracle, g2, xs, ks, table, True, threads=16)).all():
            bad.append(tag + "shard shared list")
    return bad


if __name__ == "__main__":
    # python gmsm_cases.py DEV [DEV ...]
    import oracle_lib
    from gopairingbasedcryptography_amd import bn254 as engine
    oracle_lib.build()
    engine.init([int(d) for d in sys.argv[1:]])
    failures = shard_run(engine, oracle_lib)
    print("devices", engine.num_devices(), "failures", failures)
    sys.exit(1 if failures else 0)
