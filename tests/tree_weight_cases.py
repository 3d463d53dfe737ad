"""Inputs and expectations of the threshold-tree weight tests (tests/test_fr_tree_weights.py on the CPU harness,
tests/test_fr_tree_weights_gpu.py on the device): the trees of share_cases.tree_cases() and two that take the paths those leave out (the
large LDS instance; the largest tree the handle accepts), held patterns per tree, and as the one expectation the existing
bsw07.decrypt_plan in Python integers — AccessTreeNode.DecryptNode's choice (the first `threshold` satisfied children in child order) with
the Lagrange coefficients multiplied down each path — scattered to a k x L row; a None plan is ok = 0 and a zero row.  decrypt_plan works
on attribute sets, so every tree is rebuilt with leaf y carrying the attribute y: a held mask and an attribute set are then the same thing.
Every comparison is exact."""
import zlib

import numpy as np

import fr_cases as fc
import share_cases as sc
from gopairingbasedcryptography_amd import bsw07

R = fc.R
Leaf, Threshold = bsw07.Leaf, bsw07.Threshold
BYTES = (0x01, 0x80, 0xFF)                     # what a held leaf's byte is, by item: only "non-zero" counts


def relabel(tree):
    """(the same tree with leaf y carrying attribute y and its leaf ids assigned, L)"""
    n = [0]

    def walk(t):
        if isinstance(t, Leaf):
            n[0] += 1
            return Leaf(n[0] - 1)
        return Threshold(t.k, *[walk(c) for c in t.children])
    t = walk(tree)
    bsw07.assign_leaf_ids(t)
    return t, n[0]


def many_gates():
    """2-of-16 over 2-of-16 over 2-of-2: 273 gates and 512 leaves, 3515 words per item — the large LDS instance"""
    return Threshold(2, *[Threshold(2, *[Threshold(2, Leaf(0), Leaf(1)) for _ in range(16)]) for _ in range(16)])


def largest():
    """1024 gates, 1024 leaves, a gate of 1024 children: 1023 1-of-1 gates and a leaf under a 3-of-1024 root (12289 words, the limit)"""
    return Threshold(3, *([Threshold(1, Leaf(0)) for _ in range(1023)] + [Leaf(1)]))


def trees():
    """[(label, tree with leaf y = attribute y, L)]"""
    out = [(c["label"], c["tree"]) for c in sc.tree_cases()] + [("many-gates", many_gates()), ("largest", largest())]
    return [(label,) + relabel(t) for label, t in out]


# ------------------------------------------------------------------------------------------------ held patterns
def pick_first(t):
    return list(range(t.k))


def pick_last(t):
    return list(range(len(t.children) - t.k, len(t.children)))


def pick_strided(t):
    n = len(t.children)
    return sorted(sorted(range(n), key=lambda i: (i * 7 + 3) % n)[:t.k])


def pick_over(t):
    """the last `threshold` children and the first one: one more than needed wherever the gate has it (the first-k rule drops the last)"""
    return sorted(set(pick_last(t)) | {0})


def satisfy(t, pick, short=0):
    """the leaves that satisfy exactly the children pick(gate) of every gate on the way down (`short` fewer at this gate)"""
    if isinstance(t, Leaf):
        return {t.attribute}
    idx = pick(t)
    return set().union(*[satisfy(t.children[i], pick) for i in idx[:len(idx) - short]]) if idx[:len(idx) - short] else set()


def under_unsatisfied(t, top=True):
    """every gate below the root holds one child fewer than it needs (so it is unsatisfied, with held leaves under it wherever its
    threshold is above 1); the root's own leaves are held"""
    if isinstance(t, Leaf):
        return {t.attribute}
    if top:
        return set().union(*[under_unsatisfied(c, False) for c in t.children])
    return satisfy(t, pick_first, short=1)


def patterns(tree, L):
    """[(name, set of held leaves)]"""
    every = set(range(L))
    p = [("all", every), ("first", satisfy(tree, pick_first)), ("none", set()), ("last", satisfy(tree, pick_last)), ("strided", satisfy(tree, pick_strided)),
         ("root-short", satisfy(tree, pick_first, short=1)), ("over", satisfy(tree, pick_over)), ("under-unsatisfied", under_unsatisfied(tree)),
         ("all-but-first", every - {0}), ("all-but-last", every - {L - 1}), ("even", set(range(0, L, 2)))]
    return p


def _mask(held, L, byte):
    m = np.zeros(L, dtype=np.uint8)
    m[sorted(held)] = byte
    return m


def _case(label, tree, L, k, rows):
    return {"label": label, "tree": tree, "nodes": sc.node_array(sc.preorder(tree)), "L": L, "k": k, "held": np.stack(rows)}


HEAVY = 256                                     # a flat gate this wide costs the CPU harness 0.1 s and more per item: three items a case
ITEMS = {"leaf": 130, "1-of-1": 3, "1-of-5": 130, "2-of-2": 65, "1-of-2": 1, "3-of-3": 130, "2-of-3": 65, "example": 130, "chain8": 65, "alternating": 130,
         "3of5-2of3": 65, "16x16": 130, "many-gates": 11}                     # every other tree: 65


_CASES = []


def cases():
    """the case list, built once (callers leave it as it is)"""
    if not _CASES:
        _CASES.extend(_build_cases())
    return _CASES


def _build_cases():
    """Item counts 1, 3, 65 and 130 (three workgroups of 64 items and fewer, satisfied and unsatisfied items side by side).  A light tree
    is one case: its patterns in turn, then seeded random masks of three densities.  The flat gates of 256 children come three items a
    case; the trees of 1024 children one item a case.  16x16 at 130 items is the largest launch: 130 x 256 leaves."""
    out = []
    for label, tree, L in trees():
        pats = patterns(tree, L)
        flat = not isinstance(tree, Leaf) and len(tree.children) >= HEAVY
        if flat and len(tree.children) > HEAVY:                               # 1024 children
            names = {"1-of-1024": ("last", "all"), "1024-of-1024": ("all", "root-short"), "largest": ("all", "strided", "root-short", "all-but-first")}[label]
            for i, name in enumerate(names):
                out.append(_case("%s/%s" % (label, name), tree, L, 1, [_mask(dict(pats)[name], L, BYTES[i % 3])]))
            continue
        if flat:
            for i in range(0, len(pats), 3):
                out.append(_case("%s/%d" % (label, i // 3), tree, L, len(pats[i:i + 3]), [_mask(h, L, BYTES[(i + j) % 3]) for j, (_, h) in enumerate(pats[i:i + 3])]))
            continue
        k = ITEMS.get(label, 65)
        rng = np.random.default_rng(zlib.crc32(label.encode()))
        rows = []
        for j in range(k):
            if j < len(pats):
                rows.append(_mask(pats[j][1], L, BYTES[j % 3]))
            else:
                rows.append(((rng.random(L) < (0.5, 0.8, 0.95)[j % 3]) * BYTES[j % 3]).astype(np.uint8))
        out.append(_case(label, tree, L, k, rows))
    return out


# ------------------------------------------------------------------------------------------------ expectations
_CACHE = {}


def expected_row(label, tree, L, mask):
    """(L weights, ok) of one item from bsw07.decrypt_plan"""
    key = (label.split("/")[0], (np.asarray(mask) != 0).tobytes())
    if key not in _CACHE:
        plan = bsw07.decrypt_plan(tree, {y for y in range(L) if mask[y]})
        row = [0] * L
        for leaf_id, (_, delta) in (plan or {}).items():
            row[leaf_id - 1] = delta
        _CACHE[key] = (tuple(row), int(plan is not None))
    return _CACHE[key]


def expected(c):
    """(k x L weights as Python ints, row by row; k ok flags)"""
    got = [expected_row(c["label"], c["tree"], c["L"], m) for m in c["held"]]
    return [v for row, _ in got for v in row], [ok for _, ok in got]


def run_cases(call, cases_):
    """call(case) -> (k x L scalar rows, k ok bytes); returns the labels that differ"""
    bad = []
    for c in cases_:
        w, ok = call(c)
        want_w, want_ok = expected(c)
        if fc.ints(w) != want_w or [int(v) for v in np.asarray(ok).reshape(-1)] != want_ok:
            bad.append(c["label"])
    return bad


# ------------------------------------------------------------------------------------------------ node lists in another order
# gpbc_share_tree_create asks for parent < child and no more, so the children of two gates may alternate in the list.  Leaves and gates
# are numbered in LIST order there (and a gate's coefficients follow its gate number), which is then not the order of a depth-first walk.
ROOT = sc.ROOT_MARK
OTHER_ORDERS = {
    "two gates, children alternating": [(ROOT, 2), (0, 1), (0, 1), (1, 0), (2, 0), (1, 0), (2, 0)],
    "three levels, children alternating": [(ROOT, 2), (0, 2), (0, 0), (1, 0), (0, 2), (1, 2), (4, 0), (5, 0), (4, 0), (5, 0), (1, 0)],
    "level order": [(ROOT, 2), (0, 2), (0, 1), (0, 2), (1, 0), (2, 0), (3, 0), (1, 0), (2, 0), (3, 0), (1, 0), (3, 0)],
}


def tree_of_list(nodes):
    """(tree, L, gate numbers by node): the Leaf / Threshold tree of a node list, children in list order, leaf attribute = its number in
    the list"""
    built, leaves, gates, number = [], 0, 0, {}
    for i, (_, t) in enumerate(nodes):
        if t:
            g = Threshold.__new__(Threshold)
            g.k, g.children = t, []
            built.append(g)
            number[i], gates = gates, gates + 1
        else:
            built.append(Leaf(leaves))
            leaves += 1
    for i, (parent, _) in enumerate(nodes):
        if i:
            built[parent].children.append(built[i])
    bsw07.assign_leaf_ids(built[0])
    return built[0], leaves, {id(built[i]): g for i, g in number.items()}


def list_expected(nodes, mask):
    """(L weights in list leaf order, ok) from bsw07.decrypt_plan"""
    tree, L, _ = tree_of_list(nodes)
    plan = bsw07.decrypt_plan(tree, {y for y in range(L) if mask[y]})
    row = [0] * L
    for attribute, delta in (plan or {}).values():
        row[attribute] = delta
    return row, int(plan is not None)


def list_share(nodes, secret, coeffs):
    """ShareSecret over a node list: the shares in list leaf order; gate g (list order) owns the coefficients behind those of the gates before it"""
    tree, L, gate_no = tree_of_list(nodes)
    thresholds = [t for _, t in nodes if t]
    first = [sum(t - 1 for t in thresholds[:g]) for g in range(len(thresholds))]
    out = [0] * L

    def walk(node, value):
        if isinstance(node, Leaf):
            out[node.attribute] = value % R
            return
        g = gate_no[id(node)]
        q = [value] + list(coeffs[first[g]:first[g] + node.k - 1])
        for i, c in enumerate(node.children, start=1):
            walk(c, sc.horner(q, i))
    walk(tree, secret)
    return out


def all_masks(L):
    return np.array([[(m >> y) & 1 for y in range(L)] for m in range(1 << L)], dtype=np.uint8)
