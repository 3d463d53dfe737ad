"""The cases of the formula entries (include/gpbc_bn254_formula.h) and what they must give, for the CPU harness and the GPU alike.

The expectation is a restatement of its own, in Python integers and by recursion over nested tuples ("and", l, r) / ("or", l, r) / int,
written from the header's rule and from access/lsss/lewko_waters_lsss_matrix.go:34-87; it shares nothing with formula.py (which walks
code rows with a stack) or with the kernels.  The encoder below is this file's own too.

A build case: label, nodes [k, N], rows, cols, trees (a nested formula per item, None for a malformed row).
A select case: label, nodes [k, N] or [1, N], rows, held [k, rows], trees (per item; one tree for a shared formula)."""
import itertools

import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
AND, OR, END = -2, -3, -1
INT64_MIN = -(1 << 63)
TOP = (1 << 63) - 1


# ------------------------------------------------------------------------------------------------ the restatement
def is_leaf(t):
    return not isinstance(t, tuple)


def matrix_of(tree):
    """(rows of entries in {0, 1, -1}, rho) by the reference's recursion"""
    counter, rows, rho = [1], [], []

    def visit(node, vector):
        if is_leaf(node):
            rows.append(list(vector))
            rho.append(node)
            return
        op, left, right = node
        if op == "or":
            lv, rv = list(vector), list(vector)
        else:
            c = counter[0]
            lv = [0] * c + [-1]
            rv = list(vector) + [0] * (c - len(vector)) + [1]
            counter[0] = c + 1
        visit(left, lv)
        visit(right, rv)
    visit(tree, [1])
    return [r + [0] * (counter[0] - len(r)) for r in rows], rho


def n_leaves(tree):
    return 1 if is_leaf(tree) else n_leaves(tree[1]) + n_leaves(tree[2])


def choose(tree, held):
    """(ok, chosen leaf numbers): held is indexed by leaf number in preorder"""
    def sat(node, first):
        if is_leaf(node):
            return bool(held[first])
        l, r = sat(node[1], first), sat(node[2], first + n_leaves(node[1]))
        return (l and r) if node[0] == "and" else (l or r)

    def take(node, first, out):
        if is_leaf(node):
            out.append(first)
        elif node[0] == "and":
            take(node[1], first, out)
            take(node[2], first + n_leaves(node[1]), out)
        elif sat(node[1], first):
            take(node[1], first, out)
        else:
            take(node[2], first + n_leaves(node[1]), out)
    if not sat(tree, 0):
        return False, []
    out = []
    take(tree, 0, out)
    return True, out


def well_formed(row):
    """the header's rule, entry by entry"""
    need, ended = 1, False
    for c in [int(v) for v in row]:
        if ended:
            if c != END:
                return False
            continue
        if c == END or c < OR:
            return False
        need += 1 if c < 0 else -1
        ended = need == 0
    return ended


# ------------------------------------------------------------------------------------------------ encoding
def preorder(tree):
    if is_leaf(tree):
        return [tree]
    return [AND if tree[0] == "and" else OR] + preorder(tree[1]) + preorder(tree[2])


def node_rows(trees, N):
    out = np.full((len(trees), N), END, dtype=np.int64)
    for t, tree in enumerate(trees):
        codes = preorder(tree)
        out[t, :len(codes)] = codes
    return out


def scalar(v):
    return np.frombuffer((v % R).to_bytes(32, "little"), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ trees
def shapes(n):
    """every binary tree shape with n leaves (None marks a leaf)"""
    if n == 1:
        return [None]
    return [(l, r) for i in range(1, n) for l in shapes(i) for r in shapes(n - i)]


def all_formulas(n, first=10):
    """every formula with n leaves over {and, or}; the leaves carry first, first + 1, ... in order"""
    out = []
    for shape in shapes(n):
        gates = n - 1
        for ops in itertools.product(("and", "or"), repeat=gates):
            it, leaf = iter(ops), iter(range(first, first + n))

            def fill(s):
                if s is None:
                    return next(leaf)
                op = next(it)
                l = fill(s[0])
                return (op, l, fill(s[1]))
            out.append(fill(shape))
    return out


def deep(op, n, left):
    t = 100
    for i in range(1, n):
        t = (op, t, 100 + i) if left else (op, 100 + i, t)
    return t


def balanced(n, first=0, level=0):
    if n == 1:
        return 1000 + first
    h = n // 2
    return ("and" if level % 2 == 0 else "or", balanced(h, first, level + 1), balanced(n - h, first + h, level + 1))


def random_tree(n, rng, attrs=40):
    if n == 1:
        return int(rng.integers(0, attrs))
    i = int(rng.integers(1, n))
    return ("and" if rng.integers(0, 2) else "or", random_tree(i, rng, attrs), random_tree(n - i, rng, attrs))


UP_TO_4 = [f for n in (1, 2, 3, 4) for f in all_formulas(n)]                       # 1 + 2 + 8 + 40
BIG = [deep("and", 64, True), deep("and", 64, False), deep("or", 64, False), deep("or", 64, True), balanced(64)]


def ragged():
    rng = np.random.default_rng(29)
    sizes = list(range(1, 65)) + [64, 33, 2]
    return [random_tree(n, rng) for n in sizes]                                    # k = 67


MALFORMED = [
    ("gate last", [AND, 1, OR, 2, 3, 4, AND]),
    ("gate as the only node", [OR, END, END, END, END, END, END]),
    ("END inside", [AND, 1, END, 2, END, END, END]),
    ("code behind the end", [OR, 1, 2, END, 3, END, END]),
    ("gate behind the end", [5, AND, END, END, END, END, END]),
    ("code -4", [AND, -4, 2, END, END, END, END]),
    ("INT64_MIN", [INT64_MIN, END, END, END, END, END, END]),
    ("INT64_MIN behind the end", [OR, 1, 2, INT64_MIN, END, END, END]),
    ("END only", [END] * 7),
    ("unfinished", [AND, AND, 1, 2, END, END, END]),
]


def build_cases():
    cases = [
        dict(label="one-leaf/n1", trees=[7], N=1, rows=1, cols=1),
        dict(label="one-leaf/n7", trees=[7], N=7, rows=3, cols=2),
        dict(label="or", trees=[("or", 1, 2)], N=3, rows=2, cols=1),
        dict(label="and", trees=[("and", 1, 2)], N=3, rows=2, cols=2),
        dict(label="up-to-4", trees=UP_TO_4, N=7, rows=4, cols=4),
        dict(label="up-to-4/wide", trees=UP_TO_4, N=9, rows=5, cols=7),
        dict(label="big", trees=BIG, N=127, rows=64, cols=64),
        dict(label="ragged/64x64", trees=ragged(), N=127, rows=64, cols=64),
        dict(label="ragged/16x8", trees=ragged(), N=127, rows=16, cols=8),
        dict(label="attributes", trees=[("and", 0, TOP), ("or", TOP, 0), TOP, 0], N=3, rows=2, cols=2),
        dict(label="repeated", trees=[("and", 5, 5), ("or", 5, 5), ("and", ("or", 5, 5), 5)], N=5, rows=3, cols=2),
    ]
    for c in cases:
        c["nodes"] = node_rows(c["trees"], c["N"])
    good = [("and", 1, ("or", 2, 3)), 9]
    rows = [preorder(good[0]) + [END, END]] + [r for _, r in MALFORMED] + [[9] + [END] * 6]
    cases.append(dict(label="malformed", trees=[good[0]] + [None] * len(MALFORMED) + [good[1]], N=7, rows=4, cols=3, nodes=np.array(rows, dtype=np.int64)))
    return cases


def expected_build(c):
    """(matrix [k, rows, cols, 32], rho [k, rows], dims [k, 2], ok [k])"""
    k, rows, cols = len(c["trees"]), c["rows"], c["cols"]
    matrix, rho = np.zeros((k, rows, cols, 32), dtype=np.uint8), np.full((k, rows), -1, dtype=np.int64)
    dims, ok = np.zeros((k, 2), dtype=np.int64), np.zeros(k, dtype=np.uint8)
    one, minus = scalar(1), scalar(-1)
    for t, tree in enumerate(c["trees"]):
        if tree is None:
            continue
        m, a = matrix_of(tree)
        if len(m) > rows or len(m[0]) > cols:
            continue
        ok[t], dims[t] = 1, (len(m), len(m[0]))
        rho[t, :len(a)] = a
        for x, row in enumerate(m):
            for y, v in enumerate(row):
                if v:
                    matrix[t, x, y] = one if v == 1 else minus
    return matrix, rho, dims, ok


def select_cases():
    rng = np.random.default_rng(31)
    cases = []
    trees, held = [], []
    for f in UP_TO_4:                                                             # every held subset of every formula
        n = n_leaves(f)
        for bits in itertools.product((0, 1), repeat=n):
            trees.append(f)
            held.append(list(bits) + [0] * (4 - n))
    cases.append(dict(label="up-to-4/every-subset", trees=trees, N=7, rows=4, held=np.array(held, dtype=np.uint8)))
    big_held = []
    for variant in range(4):
        for _ in BIG:
            h = np.ones(64, dtype=np.uint8)
            if variant == 1:
                h[63] = 0
            elif variant == 2:
                h[:] = 0
                h[63] = 0x80                                                      # any non-zero byte holds
            elif variant == 3:
                h = (rng.integers(0, 4, 64) > 0).astype(np.uint8)
            big_held.append(h)
    cases.append(dict(label="big", trees=BIG * 4, N=127, rows=64, held=np.array(big_held)))
    rag = ragged()
    h64 = (rng.integers(0, 3, (len(rag), 64)) > 0).astype(np.uint8)               # bytes behind an item's leaves hold anything
    cases.append(dict(label="ragged/64", trees=rag, N=127, rows=64, held=h64))
    cases.append(dict(label="ragged/16", trees=rag, N=127, rows=16, held=np.ascontiguousarray(h64[:, :16])))
    rep = [("and", 5, 5), ("or", 5, 5), ("or", 5, 5), ("or", 5, 5), ("and", ("or", 5, 5), 5), ("and", ("or", 5, 5), 5)]
    cases.append(dict(label="repeated", trees=rep, N=5, rows=3, held=np.array([[1, 1, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [0, 1, 1], [1, 1, 0]], dtype=np.uint8)))
    shared = ("or", ("and", 1, 2), ("and", 3, ("or", 4, 1)))
    cases.append(dict(label="shared/k130", trees=[shared], N=9, rows=6, shared=True, held=(rng.integers(0, 2, (130, 6))).astype(np.uint8)))
    cases.append(dict(label="shared/k1", trees=[shared], N=9, rows=5, shared=True, held=np.array([[0, 0, 1, 0, 1]], dtype=np.uint8)))
    for c in cases:
        c["nodes"] = node_rows(c["trees"], c["N"])
    bad = [preorder(("and", 1, ("or", 2, 3))) + [END, END]] + [r for _, r in MALFORMED]
    cases.append(dict(label="malformed", trees=[("and", 1, ("or", 2, 3))] + [None] * len(MALFORMED), N=7, rows=4, nodes=np.array(bad, dtype=np.int64),
                      held=np.ones((len(bad), 4), dtype=np.uint8)))
    for c in cases:
        c.setdefault("shared", False)
    return cases


def expected_select(c):
    """(chosen [k, rows], ok [k])"""
    k, rows = len(c["held"]), c["rows"]
    chosen, ok = np.zeros((k, rows), dtype=np.uint8), np.zeros(k, dtype=np.uint8)
    for j in range(k):
        tree = c["trees"][0 if c["shared"] else j]
        if tree is None or n_leaves(tree) > rows:
            continue
        good, which = choose(tree, c["held"][j])
        if good:
            ok[j] = 1
            chosen[j, which] = 1
    return chosen, ok


def by_label(cases, label):
    return next(c for c in cases if c["label"] == label)
