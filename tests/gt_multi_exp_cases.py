"""Case lists of the segmented GT multi-exponentiation, shared by the CPU harness test (test_gt_multi_exp.py) and the GPU tests
(test_gt_multi_exp_gpu.py): bases, exponents, segment tables, and the expected bytes from the oracle (gt_exp per factor, folded
with gt_mul from the left, starting at one).

The plan the cases aim at (csrc/segred29.hip.hpp with the shape of csrc/gtmexp29.hip.hpp): a call of n factors in n_seg segments cuts every segment into
J = max(1, min(n // n_seg // 4, ceil(65536 / n_seg))) pieces (product only: // 8), a lane pair takes the factors of its piece four
at a time, and the J piece values of every segment are folded by the product-only form of the same plan.  So the boundaries are:
group length 4 (3 / 4 / 5 factors), J stepping 1 -> 2 at 8 factors per segment (7 / 8 / 9; product only: 15 / 16 / 17), a second
fold level from 16 pieces on (63 / 64 / 65 factors; product only 127 / 128 / 129), and 65536 pieces per launch (GPU cases only).

Run as a script it sends the cases and three larger calls through the host-pointer entry in a process of its own bound to the device
list given on the command line (a device may be listed twice, so one GPU still crosses the shard split, which cuts by whole segments)."""
import os
import sys

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle")]

import numpy as np  # noqa: E402

import bn254_py as o  # noqa: E402

R = o.R
GT = 384
GROUP, PROD_MIN, FILL = 4, 8, 65536
SEG_LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 64, 65]
EDGE_EXPS = [0, 1, 2, 15, 16, R - 1, R, R + 1, 1 << 255, (1 << 256) - 1, int("f" * 64, 16)] + [((w * 7) % 15 + 1) << (4 * w) for w in range(64)]


def pieces(n, n_seg, has_k):
    """segred_pieces (csrc/segred29.hip.hpp) with GT_MEXP_SHAPE, restated"""
    return max(1, min(n // n_seg // (GROUP if has_k else PROD_MIN), -(-FILL // n_seg)))


def krows(ks):
    return np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in ks), dtype=np.uint8).reshape(-1, 32).copy()


def rand_exps(tag, n):
    rng = np.random.default_rng(abs(hash_tag(tag)))
    return [int.from_bytes(rng.bytes(32), "little") for _ in range(n)]


def hash_tag(tag):
    import hashlib
    return int.from_bytes(hashlib.sha256(tag.encode()).digest()[:4], "little")


_POOL = {}


def pool(oracle):
    """'pair': 12 pairing values (cyclotomic); 'miller': 3 Miller values (not cyclotomic); 'one'; 'inv': the inverses of 'pair'"""
    if not _POOL:
        P = np.frombuffer(b"".join(o.g1_to_bytes(o.g1_mul(o.G1_GEN, 1000 + 17 * i)) for i in range(12)), dtype=np.uint8)
        Q = np.frombuffer(b"".join(o.g2_to_bytes(o.g2_mul(o.G2_GEN, 77 + 5 * i)) for i in range(12)), dtype=np.uint8)
        _POOL["pair"] = oracle.pair_batch(P, Q)
        _POOL["miller"] = oracle.miller_loop(P[:3 * 64], Q[:3 * 128])
        _POOL["one"] = oracle.gt_exp(_POOL["pair"][:1], krows([0]))
        _POOL["inv"] = oracle.gt_inverse(_POOL["pair"])
        assert (oracle.gt_mul(_POOL["pair"], _POOL["inv"]) == _POOL["one"][0]).all()
    return _POOL


def take(rows, n, start=0):
    return np.stack([rows[(start + i) % len(rows)] for i in range(n)]) if n else np.zeros((0, GT), dtype=np.uint8)


def offsets(lengths):
    return [0] + list(np.cumsum(lengths).astype(int))


def cases(oracle):
    """(label, x[n, 384], k (list of n or of m integers, or None), seg_off (list), shared)"""
    p = pool(oracle)
    pair, miller, one, inv = p["pair"], p["miller"], p["one"], p["inv"]
    out = []
    # every length as a call of its own (one segment) and all of them in one call, random exponents
    for L in SEG_LENGTHS + [7, 8, 9, 63]:
        out.append(("one segment of %d" % L, take(pair, L, L), rand_exps("len%d" % L, L), [0, L], False))
    n = sum(SEG_LENGTHS)
    out.append(("all lengths in one call", take(pair, n), rand_exps("all", n), offsets(SEG_LENGTHS), False))
    out.append(("all lengths, reversed, empty segments at both ends", take(pair, n, 3), rand_exps("rev", n), offsets([0] + SEG_LENGTHS[::-1] + [0]), False))
    # the edge exponents: each alone (one-element segments), then as the factors of segments of 5 (75 = 15 x 5)
    E = EDGE_EXPS
    out.append(("edge exponents, one per segment", take(pair, len(E)), E, list(range(len(E) + 1)), False))
    out.append(("edge exponents, segments of 5", take(pair, len(E), 5), E, list(range(0, len(E) + 1, 5)), False))
    out.append(("all exponents zero", take(pair, 9), [0] * 9, [0, 4, 9], False))
    # bases
    out.append(("one as a base", np.concatenate([one, pair[:2], one, one]), rand_exps("one", 5), [0, 1, 4, 5], False))
    out.append(("a base and its inverse", np.stack([pair[0], inv[0], pair[1], pair[2], inv[2], inv[1]]), [5, 5, R + 3, 1 << 200, 1 << 200, R + 3], [0, 2, 6], False))
    out.append(("the same base through a segment", take(pair[3:4], 17), rand_exps("same", 17), [0, 17], False))
    out.append(("a Miller value alone", miller[:1], [(1 << 256) - 1], [0, 1], False))
    out.append(("Miller values only", take(miller, 6), rand_exps("mil", 6), [0, 1, 6], False))
    out.append(("Miller and pairing values mixed", np.stack([pair[0], miller[0], pair[1], pair[2], pair[3], miller[1], pair[4], pair[5], pair[6]]),
                EDGE_EXPS[5:11] + rand_exps("mix", 3), [0, 3, 3, 9], False))
    # the shared exponent list (nk = m for segments of m) and the plain product (k = None)
    for m, segs in ((1, 3), (4, 3), (5, 2), (16, 2), (9, 1)):
        out.append(("shared list of %d for %d segments" % (m, segs), take(pair, m * segs, m), rand_exps("sh%d" % m, m), list(range(0, m * segs + 1, m)), True))
    out.append(("shared edge exponents", take(pair, 22, 1), EDGE_EXPS[:11], [0, 11, 22], True))
    for L in (0, 1, 2, 7, 8, 9, 15, 16, 17, 65, 127, 128, 129):
        out.append(("product of %d" % L, take(pair, L, L), None, [0, L], False))
    out.append(("products, all lengths", take(np.concatenate([pair, miller, one]), n), None, offsets(SEG_LENGTHS), False))
    out.append(("product of a base and its inverse", np.stack([pair[0], inv[0], miller[0]]), None, [0, 2, 3], False))
    return out


def expect(oracle, x, k, seg, shared):
    one = pool(oracle)["one"][0]
    n_seg = len(seg) - 1
    if k is None:
        e = x
    else:
        ks = list(k) * n_seg if shared else k
        e = oracle.gt_exp(x, krows(ks)) if len(x) else x
    out = np.zeros((n_seg, GT), dtype=np.uint8)
    for s in range(n_seg):
        acc = one
        for i in range(seg[s], seg[s + 1]):
            acc = oracle.gt_mul(acc, e[i])[0]
        out[s] = acc
    return out


def run_engine_cases(eng, oracle, put=None, table_on_device=False):
    """every case through eng.gt_multi_exp (k = None: also eng.gt_prod): numpy arrays, or with put = a host-to-device function CUDA
    tensors, the segment table on the host or on the device.  Returns the list of failures."""
    bad = []
    for label, x, k, seg, shared in cases(oracle):
        want = expect(oracle, x, k, seg, shared)
        xs = np.ascontiguousarray(x).reshape(-1)
        kk = None if k is None else krows(k).reshape(-1)
        if put is None:
            got = eng.gt_multi_exp(xs, kk, seg)
            alt = eng.gt_prod(xs, seg) if k is None else got
        else:
            table = put(np.array(seg, dtype=np.int64)) if table_on_device else seg
            got = eng.gt_multi_exp(put(xs), None if kk is None else put(kk), table).cpu().numpy()
            alt = eng.gt_prod(put(xs), table).cpu().numpy() if k is None else got
        if not (np.asarray(got).reshape(-1, GT) == want).all() or not (np.asarray(alt).reshape(-1, GT) == want).all():
            bad.append(label)
    return bad


def ragged_case(oracle, n_seg, tag):
    """n_seg segments of lengths 0 .. 5 in a fixed irregular order over pool bases with random exponents: (x, k, seg)"""
    p = pool(oracle)
    lengths = [(7 * i + i // 5) % 6 for i in range(n_seg)]
    seg = offsets(lengths)
    n = seg[-1]
    rows = np.concatenate([p["pair"], p["miller"][:1]])
    x = rows[np.arange(n) % len(rows)]
    return x, rand_exps(tag, n), seg


def expect_threads(oracle, x, k, seg, shared, threads=16):
    """expect() for thousands of factors: the exponentiations on `threads` oracle threads"""
    n_seg = len(seg) - 1
    e = x if k is None else oracle.gt_exp(x, krows(list(k) * n_seg if shared else k), threads=threads)
    one = pool(oracle)["one"][0]
    out = np.zeros((n_seg, GT), dtype=np.uint8)
    for s in range(n_seg):
        acc = one
        for i in range(seg[s], seg[s + 1]):
            acc = oracle.gt_mul(acc, e[i])[0]
        out[s] = acc
    return out


def shard_run(eng, oracle):
    """host-pointer calls large enough for the shard split (whole segments per shard, tables rebased): ragged segments with one
    exponent per element, equal segments with a shared list, plain products; plus the case list on the smaller routes"""
    bad = run_engine_cases(eng, oracle)
    x, k, seg = ragged_case(oracle, 6000, "shard-ragged")
    if not (eng.gt_multi_exp(x.reshape(-1), krows(k).reshape(-1), seg) == expect_threads(oracle, x, k, seg, False)).all():
        bad.append("shard ragged")
    if not (eng.gt_prod(x.reshape(-1), seg) == expect_threads(oracle, x, None, seg, False)).all():
        bad.append("shard products")
    m, segs = 3, 3000
    xs = x[:m * segs]
    ks = rand_exps("shard-shared", m)
    table = list(range(0, m * segs + 1, m))
    if not (eng.gt_multi_exp(xs.reshape(-1), krows(ks).reshape(-1), table) == expect_threads(oracle, xs, ks, table, True)).all():
        bad.append("shard shared list")
    return bad


if __name__ == "__main__":
    # python gt_multi_exp_cases.py DEV [DEV ...]
    import oracle_lib
    from gopairingbasedcryptography_amd import bn254 as engine
    oracle_lib.build()
    engine.init([int(d) for d in sys.argv[1:]])
    failures = shard_run(engine, oracle_lib)
    print("devices", engine.num_devices(), "failures", failures)
    sys.exit(1 if failures else 0)
