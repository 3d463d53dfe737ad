"""Test helper: the case corpus of the indexed fixed-base sums and of LSSS share generation (include/gpbc_bn254_indexed.h), with what
they must give — shares in Python integers, points from oracle_lib: one scalar multiplication per term on the selected base and the
oracle's sum per output.  Shared by the host-harness test (test_indexed_lane.py) and the GPU tests; an expectation is computed once
per case and kept."""
import random

import numpy as np

import bn254_py as o

R = o.R
TOP = (1 << 256) - 1
NONE = 0xFFFFFFFF
SPECIAL = [0, 1, R - 1, R, R + 1, TOP]
G1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
G2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)


def rows(vals):
    """ints below 2^256, NOT reduced -> [n, 32] scalar rows"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


def ints(buf):
    return [int.from_bytes(r.tobytes(), "little") for r in np.asarray(buf, dtype=np.uint8).reshape(-1, 32)]


# ------------------------------------------------------------------------------------------------ indexed sums
NBASE = 6
INF_BASE, EQUAL_BASES = 2, (1, 4)
_bases = {}


def bases(oracle, g2):
    """six bases: base 2 is the point at infinity, bases 1 and 4 are equal"""
    if g2 not in _bases:
        ks = [o.bench_scalar("indexed-base", i) for i in range(NBASE)]
        ks[EQUAL_BASES[1]] = ks[EQUAL_BASES[0]]
        b = np.asarray((oracle.g2_scalar_mul if g2 else oracle.g1_scalar_mul)(G2 if g2 else G1, rows(ks), threads=4)).copy()
        b[INF_BASE] = 0
        _bases[g2] = b
    return _bases[g2]


def indexed_case(n, terms, n_index_rows, seed=0, invalid=True):
    """{index [P, terms] uint32, scalars: n x terms ints, n, terms, P, planted: names of what was planted}.  Random indices (one in eight
    NONE) and scalars, then the corpus planted output by output: the special scalars anywhere; patterns that need particular indices only
    when there are enough index rows to give each its own (P >= 16), an index row being shared by the outputs i = row (mod P)."""
    rnd = random.Random(1000 * n + 10 * terms + n_index_rows + seed)
    P = n_index_rows
    index = [[NONE if rnd.randrange(8) == 0 else rnd.randrange(NBASE) for _ in range(terms)] for _ in range(P)]
    scalars = [[rnd.randrange(R) for _ in range(terms)] for _ in range(n)]
    planted = []
    for i, v in enumerate(SPECIAL):                                       # special scalars, on a finite base when the row is ours to set
        if i < n:
            scalars[i][0] = v
            if P >= 16:
                index[i % P][0] = 0 if i % 2 else NBASE - 1               # indices 0 and nbase - 1
    planted.append("special")
    if P >= 16:
        planted.append("ends")
        at = len(SPECIAL)

        def plant(name, idx_row, ks):
            nonlocal at
            if at >= min(n, P) or len(idx_row) > terms:
                return
            index[at % P] = list(idx_row) + [NONE] * (terms - len(idx_row))
            for i in range(at, n, P):                                       # every output of the row gets the pattern's scalars
                scalars[i] = list(ks) + [rnd.randrange(R) for _ in range(terms - len(ks))]
            planted.append(name)
            at += 1
        k = rnd.randrange(2, R)
        plant("cancel", [0, 0], [k, R - k])
        plant("cancel-then-more", [3, 3, 5], [k, R - k, 7])
        plant("double", [3, 3], [k, k])
        plant("double-one", [5, 5], [1, 1])
        plant("equal-bases", list(EQUAL_BASES), [k, k])
        plant("equal-bases-cancel", list(EQUAL_BASES), [k, R - k])
        plant("all-none", [NONE] * terms, [rnd.randrange(R) for _ in range(terms)])
        plant("inf-base", [INF_BASE] * terms, [rnd.randrange(1, R) for _ in range(terms)])
        plant("zero-scalars", [1] * terms, [0] * terms)
        plant("order-scalars", [1] * terms, [R] * terms)
        if invalid:
            plant("index-nbase", [NBASE], [5])
            plant("index-fffffffe", [0xFFFFFFFE] if terms == 1 else [0, 0xFFFFFFFE], [5] * min(terms, 2))
    return {"index": np.array(index, dtype=np.uint32).reshape(P, terms), "scalars": scalars, "n": n, "terms": terms, "P": P, "planted": planted}


_expected = {}


def expected(oracle, g2, case, key=None):
    """(points [n, 64|128], ok [n]) of a case over bases(oracle, g2)"""
    if key is not None and (g2, key) in _expected:
        return _expected[(g2, key)]
    b, width = bases(oracle, g2), 128 if g2 else 64
    n, terms, P, index = case["n"], case["terms"], case["P"], case["index"]
    ok = np.ones(n, dtype=np.uint8)
    sel, ks, owner = [], [], []
    for i in range(n):
        row = [int(v) for v in index[i % P]]
        if any(v != NONE and v >= NBASE for v in row):
            ok[i] = 0
            continue
        for t, j in enumerate(row):
            k = case["scalars"][i][t] % R
            if j != NONE and j != INF_BASE and k:
                sel.append(j); ks.append(k); owner.append(i)
    out = np.zeros((n, width), dtype=np.uint8)
    if sel:
        pts = np.asarray((oracle.g2_scalar_mul if g2 else oracle.g1_scalar_mul)(b[sel].reshape(-1), rows(ks), threads=8)).reshape(-1, width)
        owner = np.array(owner)
        for i in np.unique(owner):
            out[i] = np.asarray((oracle.g2_sum if g2 else oracle.g1_sum)(pts[owner == i].reshape(-1))).reshape(width)
    if key is not None:
        _expected[(g2, key)] = (out, ok)
    return out, ok


# ------------------------------------------------------------------------------------------------ LSSS shares
SHARE_SHAPES = [(1, 1), (4, 3), (16, 15), (64, 64)]
ENTRIES = [0, 1, R - 1, R, TOP]


def shares_case(nrows, cols, k, per_item, seed=0):
    """{matrix: [nm][rows][cols] ints, vectors: [k][cols] ints, want: [k][rows] ints}: entries from {0, 1, r - 1, r, 2^256 - 1, random}"""
    rnd = random.Random(100000 * nrows + 1000 * cols + 2 * k + per_item + seed)
    draw = lambda: rnd.choice(ENTRIES) if rnd.randrange(2) else rnd.randrange(1 << 256)
    nm = k if per_item else 1
    matrix = [[[draw() for _ in range(cols)] for _ in range(nrows)] for _ in range(nm)]
    vectors = [[draw() for _ in range(cols)] for _ in range(k)]
    if k and nrows * cols > 1:
        matrix[0][nrows - 1] = [TOP] * cols                                 # the largest sum the accumulator can see
        vectors[0] = [TOP] * cols
    want = [[sum(a * b for a, b in zip(matrix[j if per_item else 0][x], vectors[j])) % R for x in range(nrows)] for j in range(k)]
    return {"matrix": matrix, "vectors": vectors, "want": want, "rows": nrows, "cols": cols, "k": k, "nm": nm}


def matrix_rows(case):
    return rows([v for m in case["matrix"] for r in m for v in r])


def vector_rows(case):
    return rows([v for r in case["vectors"] for v in r])
