"""Inputs and expectations of the LSSS-weight tests (tests/test_fr_lsss.py on the CPU harness, tests/test_fr_lsss_gpu.py on the
device).  The expectation is lw11.reconstruction_weights — Gauss-Jordan elimination in Python integers — spread over all rows of
the matrix: the weight of a row that is not held, or held and dependent on the held rows before it, is 0; a mask that does not
satisfy the policy gives ok = 0 and a zero row.  Every comparison is exact.

A case is a dict: matrices [nm][rows][cols] (nm is 1 or k), held [k][rows] of 0 / 1, k systems.  `run_cases(call, cases)` sends each
through call(matrix_scalars, nm, rows, cols, held_bytes, k), which returns (w [k * rows] scalars, ok [k] bytes).

Run as a script it sends the lists and a batch above the shard minimum through the host-pointer entry in a process of its own bound
to the device list given on the command line (a device may be listed twice, so one GPU still crosses the shard split)."""
import os
import sys

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle"), os.path.join(_root, "tests")]

import numpy as np  # noqa: E402

import fr_cases as fc  # noqa: E402
import lw11_fixture as lf  # noqa: E402
from gopairingbasedcryptography_amd import lw11  # noqa: E402

R = fc.R
SIZES = ((1, 1), (2, 2), (3, 5), (5, 3), (16, 16), (17, 4), (63, 63), (64, 64), (64, 1), (1, 64))
KS = (1, 2, 70, 1000)
WAVE = 64


def systems_per_workgroup(rows, cols):
    """fr_lsss_geometry of csrc/fr29.hip.hpp restated (tests/test_fr_lsss.py compares it with what the harness reports)"""
    gw = min(64, max(rows + 1, cols))
    words = (rows + 1) * ((cols * 9) | 1)
    block = 7424 if words <= 7424 else 20480 if words <= 20480 else 65 * 577
    return min(WAVE // gw, block // words)


def expect_one(matrix, held):
    """(weights over all rows, ok) of one system"""
    rows = len(matrix)
    rho = list(range(rows))
    got = lw11.reconstruction_weights(matrix, rho, [x for x in range(rows) if held[x]])
    w = [0] * rows
    if got is None:
        return w, 0
    for x, wx in zip(*got):
        w[x] = wx
    return w, 1


def expect(case):
    ws, oks = [], []
    for t in range(case["k"]):
        w, ok = expect_one(case["matrices"][t if len(case["matrices"]) > 1 else 0], case["held"][t])
        ws += w
        oks.append(ok)
    return ws, oks


def mk(label, matrices, held):
    rows, cols = len(matrices[0]), len(matrices[0][0])
    assert all(len(m) == rows and all(len(r) == cols for r in m) for m in matrices) and all(len(h) == rows for h in held)
    assert len(matrices) in (1, len(held))
    return {"label": label, "matrices": [[[int(v) % (1 << 256) if int(v) >= 0 else int(v) % R for v in r] for r in m] for m in matrices],
            "held": [[1 if v else 0 for v in h] for h in held], "k": len(held), "rows": rows, "cols": cols}


def rand_matrix(tag, rows, cols):
    v = fc.rand(tag, rows * cols)
    return [v[i * cols:(i + 1) * cols] for i in range(rows)]


def sparse_matrix(tag, rows, cols):
    """entries from {0, 1, -1, a random scalar}: the look of a Lewko-Waters matrix, with dependent rows and zero columns by chance"""
    v = fc.rand(tag, rows * cols)
    pick = lambda x: (0, 0, 1, R - 1, 0, x, 1, 0)[x % 8]
    return [[pick(v[i * cols + j]) for j in range(cols)] for i in range(rows)]


def rand_mask(tag, rows, k, drop=5):
    v = fc.rand(tag, rows * k)
    return [[0 if v[t * rows + x] % drop == 0 else 1 for x in range(rows)] for t in range(k)]


def size_cases():
    """every (rows, cols) of the list with a matrix per system (dense and sparse alternating, random masks), k chosen in turn from KS
    and, per size, one below, at and above the number of systems a workgroup takes"""
    out = []
    for i, (rows, cols) in enumerate(SIZES):
        spw = systems_per_workgroup(rows, cols)
        ks = {KS[i % len(KS)], max(1, spw - 1), spw, spw + 1}
        if rows * cols >= 63 * 63:
            ks = {1, 2, 3} if rows * cols > 63 * 63 else {1, 2}             # the 64 x 64 eliminations in Python integers are the slow part
        for k in sorted(ks):
            tag = "sz-%d-%d-%d" % (rows, cols, k)
            gen = sparse_matrix if (i + k) % 2 else rand_matrix
            if k >= 70:                                                     # many systems: a few matrices repeated with different masks
                base = [gen(tag + "-%d" % t, rows, cols) for t in range(7)]
                mats = [base[t % 7] for t in range(k)]
            else:
                mats = [gen(tag + "-%d" % t, rows, cols) for t in range(k)]
            out.append(mk(tag, mats, rand_mask(tag + "h", rows, k)))
    return out


def large_k_cases():
    """k = 70 and 1000 on small systems (several workgroups, a short last one)"""
    out = []
    for rows, cols, k in ((16, 16, 70), (5, 3, 1000), (3, 5, 70), (17, 4, 70)):
        tag = "lk-%d-%d-%d" % (rows, cols, k)
        base = [sparse_matrix(tag + "-%d" % t, rows, cols) for t in range(5)] + [lf.threshold_policy(min(cols, rows), rows)[0]]
        base = [[r[:cols] + [0] * (cols - len(r)) for r in m] for m in base]
        out.append(mk(tag, [base[t % len(base)] for t in range(k)], rand_mask(tag + "h", rows, k, drop=4)))
    return out


def mask_of(rho, attrs):
    return [1 if a in attrs else 0 for a in rho]


def policy_cases():
    out = []
    m, rho = lf.and_or_policy()
    sets = [{11, 22}, {33, 44}, {11, 33}, {11, 22, 33, 44}]
    out.append(mk("and-or", [m], [mask_of(rho, s) for s in sets]))
    for n in (1, 2, 16, 64):
        m, rho = lf.and_chain_policy(n)
        held = [[1] * n] + [[0 if x == j else 1 for x in range(n)] for j in sorted({0, n // 2, n - 1})]
        out.append(mk("and-chain-%d" % n, [m], held))
    for t, n in ((3, 5), (8, 16)):
        m, rho = lf.threshold_policy(t, n)
        held = [[1] * t + [0] * (n - t), [0] * (n - t) + [1] * t, [1] * n, [1] * (t - 1) + [0] * (n - t + 1), [x % 2 for x in range(n)]]
        out.append(mk("shamir-%d-of-%d" % (t, n), [m], held))
    return out


def pivot_cases():
    out = [mk("swap-needed", [[[0, 1, 0], [1, 0, 0], [0, 0, 1]]], [[1, 1, 1], [1, 1, 0], [1, 0, 1]]),
           mk("first-row-zero-in-eq0", [[[0, 5, 1], [1, 1, 0], [0, R - 5, R - 1]]], [[1, 1, 1], [0, 1, 1], [1, 1, 0]])]
    # the same vector twice in the middle (an OR gate): the second copy gets weight 0
    rep = [[1, 1, 0], [0, R - 1, 1], [0, R - 1, 1], [0, 0, R - 1], [0, 0, R - 1]]
    out.append(mk("repeated-row", [rep], [[1, 1, 1, 1, 1], [1, 0, 1, 0, 1], [1, 1, 1, 0, 0], [0, 1, 1, 1, 1]]))
    out.append(mk("nothing-held", [rep], [[0] * 5]))
    out.append(mk("zero-matrix", [[[0, 0], [0, 0]]], [[1, 1]]))
    out.append(mk("target-needs-all", [[[1, 2, 3], [0, 1, 4], [0, 0, 1]]], [[1, 1, 1], [1, 1, 0], [1, 0, 0]]))
    return out


def value_cases():
    big = (1 << 256) - 1
    out = [mk("unreduced-entries", [[[R + 1, big], [big, R + 1]], [[R + 1, 0], [0, big]], [[big, big], [1, 2]]], [[1, 1], [1, 1], [1, 1]]),
           mk("minus-one-as-r-1", [[[1, 1], [0, R - 1]]], [[1, 1], [1, 0]]),
           # equation 0 of the first unknown is exactly r (and 5 r): to be skipped as zero, the pivot is equation 1
           mk("r-where-the-pivot-search-looks", [[[R, 1], [1, 0]], [[5 * R, 1], [1, R]], [[2 * R, 3 * R], [1, 0]]], [[1, 1], [1, 1], [1, 1]]),
           # eliminating unknown 0 makes 2 * 3 - 3 * 2 = 0 in equation 1 of unknown 1 from non-zero entries: row 1 is dependent
           mk("difference-zero", [[[2, 3, 1], [4, 6, 2], [0, 1, 0], [1, 0, 0]]], [[1, 1, 1, 1], [1, 1, 0, 1], [1, 1, 1, 0], [0, 1, 1, 1]]),
           mk("difference-zero-unreduced", [[[R + 2, 3], [2 * R + 4, R + 6], [1, 0]]], [[1, 1, 1], [1, 1, 0]])]
    E = list(fc.EDGES)
    rows = 6
    em = [[E[(i * 5 + j * 3) % len(E)] for j in range(rows)] for i in range(rows)]
    out.append(mk("edge-values", [em], [[1] * rows, [1, 0, 1, 1, 0, 1]]))
    return out


def dense_cases():
    out = [mk("dense-8x8", [rand_matrix("d8", 8, 8)], [[1] * 8]),
           mk("dense-64x64", [rand_matrix("d64", 64, 64)], [[1] * 64]),
           mk("dense-wide-5x9", [rand_matrix("dw", 5, 9)], [[1] * 5]),
           mk("dense-wide-63x64", [rand_matrix("dw63", 63, 64)], [[1] * 63])]
    return out


def broadcast_cases():
    m, _ = lf.threshold_policy(3, 7)
    held = rand_mask("bc", 7, 9, drop=3)
    return [mk("one-matrix-k-masks", [m], held), mk("matrix-per-mask", [m if t % 2 else rand_matrix("bcm%d" % t, 7, 3) for t in range(9)], held)]


def all_cases():
    return size_cases() + large_k_cases() + policy_cases() + pivot_cases() + value_cases() + dense_cases() + broadcast_cases()


_EXPECT = {}


def expected(case):
    """computed once per process and shared between the tests"""
    if case["label"] not in _EXPECT:
        _EXPECT[case["label"]] = expect(case)
    return _EXPECT[case["label"]]


def flat(matrices):
    return fc.rows([v for m in matrices for r in m for v in r])


def mask_bytes(held):
    return np.array(held, dtype=np.uint8).reshape(-1)


def run_cases(call, cases):
    """the labels of the cases whose output differs from Python's"""
    bad = []
    for c in cases:
        w, ok = call(flat(c["matrices"]), len(c["matrices"]), c["rows"], c["cols"], mask_bytes(c["held"]), c["k"])
        ew, eok = expected(c)
        if fc.ints(w) != ew or [int(v) for v in np.asarray(ok).reshape(-1)] != eok:
            bad.append(c["label"])
    return bad


def satisfies(case, w, ok):
    """every ok = 1 row of w satisfies sum_x w_x M_x = e_0 with weights only on held rows, recomputed here"""
    w = fc.ints(w)
    rows, cols = case["rows"], case["cols"]
    for t in range(case["k"]):
        m = case["matrices"][t if len(case["matrices"]) > 1 else 0]
        wt = w[t * rows:(t + 1) * rows]
        if not int(ok[t]):
            if any(wt):
                return False
            continue
        if any(wx and not case["held"][t][x] for x, wx in enumerate(wt)):
            return False
        for j in range(cols):
            if sum(wx * m[x][j] for x, wx in enumerate(wt)) % R != (1 if j == 0 else 0):
                return False
    return True


def engine_call(eng, put=lambda a: a, back=lambda a: a):
    def call(m, nm, rows, cols, held, k):
        w, ok = eng.fr_lsss_weights(put(m.reshape(-1)), rows, cols, put(held))
        return np.asarray(back(w)).reshape(-1, 32), np.asarray(back(ok)).reshape(-1)
    return call


def shard_case():
    """9000 systems of 4 x 3 (the shard minimum is 2^16 / 12 = 5461 systems): the AND / OR policy and sparse matrices in turn"""
    base = [lf.and_or_policy()[0]] + [sparse_matrix("sh%d" % t, 4, 3) for t in range(6)]
    k = 9000
    return mk("shard", [base[t % 7] for t in range(k)], rand_mask("shh", 4, k, drop=4))


if __name__ == "__main__":
    # python fr_lsss_cases.py DEV [DEV ...]
    from gopairingbasedcryptography_amd import bn254 as engine
    engine.init([int(d) for d in sys.argv[1:]])
    shared = mk("shard-shared", [lf.threshold_policy(2, 3)[0]], rand_mask("shs", 3, 16000, drop=3))       # 2^16 / 6 = 10922 per shard at least
    failures = run_cases(engine_call(engine), policy_cases() + pivot_cases() + value_cases() + broadcast_cases() + [shard_case(), shared])
    print("devices", engine.num_devices(), "failures", failures)
    sys.exit(1 if failures else 0)
