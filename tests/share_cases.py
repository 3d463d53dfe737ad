"""Inputs and expectations of the secret-sharing tests (tests/test_fr_share.py on the CPU harness, tests/test_fr_share_gpu.py on the
device; the stand-in engines of the BSW07 Encrypt and SW05 KeyGenerate plan tests): the case lists of gpbc_fr_poly_eval and
gpbc_fr_share_tree and both restated in Python integers from the reference's loops — utils.ComputePolynomialValue (Horner from the top
coefficient) and the recursion of AccessTreeNode.ShareSecret (access/tree/access_tree_node.go:58-75: a gate draws threshold - 1
coefficients when it is entered, child i gets q(i), a leaf keeps its value).  Every comparison is exact."""
import functools

import numpy as np

import bn254_py as o
import fr_cases as fc
from gopairingbasedcryptography_amd import bsw07
import bsw07_fixture

R = o.R
Leaf, Threshold = bsw07.Leaf, bsw07.Threshold
ROOT_MARK = 0xFFFFFFFF
TOP = (1 << 256) - 1


def rand(tag, n):
    return [o.bench_scalar("share-" + tag, i) for i in range(n)]


# ------------------------------------------------------------------------------------------------ polynomial evaluation
def horner(coeffs, x):
    """utils.ComputePolynomialValue: from the top coefficient down"""
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def poly_expected(c):
    """k x m values, row by row"""
    pick = lambda rows, j: rows[j if len(rows) > 1 else 0]
    return [horner(pick(c["coeffs"], j), x) for j in range(c["k"]) for x in pick(c["points"], j)]


def _poly(label, d, m, k, nc=None, np_=None):
    nc, np_ = k if nc is None else nc, k if np_ is None else np_
    flat_c, flat_p = rand("c-" + label, nc * d), rand("p-" + label, np_ * m)
    return {"label": label, "d": d, "m": m, "k": k, "coeffs": [flat_c[j * d:(j + 1) * d] for j in range(nc)], "points": [flat_p[j * m:(j + 1) * m] for j in range(np_)]}


POLY_D = (1, 2, 3, 64, 65, 256, 257, 1024)
POLY_M = (1, 63, 64, 65, 256, 257, 1024)


def poly_size_cases():
    """d and m at the wave, staging-stride and LDS-instance edges (not all crossed); k = 1, 3, 65"""
    shapes = [(1, 1, 1), (1, 64, 3), (2, 63, 3), (2, 1024, 1), (3, 64, 1), (3, 65, 65), (64, 65, 3), (64, 1, 65), (65, 63, 3), (65, 256, 1), (256, 1, 3), (256, 257, 1),
              (257, 64, 3), (257, 257, 1), (1024, 63, 1), (1024, 1, 3), (16, 24, 65)]
    return [_poly("size-%d-%d-%d" % s, *s) for s in shapes]


def poly_big_case():
    return _poly("big", 1024, 1024, 1)


def poly_row_cases():
    """(n_coeff_rows, n_point_rows) in {1, k}^2, with the points of a row packed into one wave (m = 7) and spread over two workgroups (m = 70)"""
    return [_poly("rows-%d-%d-%d" % (m, nc, np_), 5, m, 3, nc, np_) for m in (7, 70) for nc in (1, 3) for np_ in (1, 3)]


def poly_value_cases():
    points = [0, 1, R - 1, R, TOP, 2, 3, 1024, R + 1, 5 * R] + rand("vp", 3)
    rows = {"zero": [0] * 6, "top-zero": rand("vtz", 5) + [0], "top-r": rand("vtr", 5) + [R], "big": [R, TOP, 5 * R + 3, R - 1, 1 << 255, TOP],
            "one": [TOP], "rand": rand("vr", 6)}
    return [{"label": "values-" + name, "d": len(row), "m": len(points), "k": 1, "coeffs": [row], "points": [points]} for name, row in rows.items()]


def poly_cases():
    return poly_size_cases() + poly_row_cases() + poly_value_cases()


def rows(values):
    return fc.rows(values).reshape(-1)


def run_poly_cases(call, cases):
    """call(coeffs bytes, n_coeff_rows, d, points bytes, n_point_rows, m, k) -> k x m scalar rows; returns the labels that differ"""
    bad = []
    for c in cases:
        got = call(rows([v for r in c["coeffs"] for v in r]), len(c["coeffs"]), c["d"], rows([v for r in c["points"] for v in r]), len(c["points"]), c["m"], c["k"])
        if fc.ints(got) != poly_expected(c):
            bad.append(c["label"])
    return bad


# ------------------------------------------------------------------------------------------------ threshold trees
def preorder(tree):
    """[(parent, threshold)] in depth-first preorder, threshold 0 for a leaf: the node list of gpbc_share_tree_create"""
    nodes = []

    def walk(node, parent):
        me = len(nodes)
        nodes.append((parent, 0 if isinstance(node, Leaf) else node.k))
        if not isinstance(node, Leaf):
            for c in node.children:
                walk(c, me)
    walk(tree, ROOT_MARK)
    return nodes


def node_array(nodes):
    return np.array(nodes, dtype=np.uint32).reshape(-1, 2)


def n_coeffs(tree):
    return 0 if isinstance(tree, Leaf) else tree.k - 1 + sum(n_coeffs(c) for c in tree.children)


def share(tree, secret, coeffs, gates=None):
    """ShareSecret: the leaf values in leaf order.  coeffs: the item's coefficients in the order the recursion draws them.
    gates (a list) receives (threshold, value, [children's values]) per gate."""
    it = iter(coeffs)
    out = []

    def walk(node, value):
        if isinstance(node, Leaf):
            out.append(value % R)
            return
        q = [value] + [next(it) for _ in range(node.k - 1)]
        vals = [horner(q, i) for i in range(1, len(node.children) + 1)]
        if gates is not None:
            gates.append((node.k, value % R, vals))
        for c, v in zip(node.children, vals):
            walk(c, v)
    walk(tree, secret)
    assert next(it, None) is None
    return out


def _tree_case(label, tree, k, secrets=None):
    C = n_coeffs(tree)
    secrets = (secrets or []) + rand("s-" + label, k)
    flat = rand("q-" + label, k * C)
    return {"label": label, "tree": tree, "k": k, "secrets": secrets[:k], "coeffs": [flat[j * C:(j + 1) * C] for j in range(k)]}


def flat_gate(k, n):
    return Threshold(k, *[Leaf(i) for i in range(n)])


def chain(depth):
    """`depth` gates, alternating 1-of-1 (one child: the next gate) and 2-of-2 (a leaf, then the next gate)"""
    node = Leaf(0)
    for lv in range(depth):
        node = Threshold(1, node) if lv % 2 else Threshold(2, Leaf(lv + 1), node)
    return node


def sixteen_by_sixteen():
    return Threshold(16, *[flat_gate(16, 16) for _ in range(16)])


def alternating():
    """children leaf / gate / leaf / gate ...: the leaves of one gate are not neighbours in the output"""
    return Threshold(4, Leaf(0), flat_gate(2, 3), Leaf(1), Threshold(2, Leaf(2), flat_gate(1, 2), Leaf(3)), Leaf(4), flat_gate(3, 3))


def three_of_five_over_two_of_three():
    return Threshold(3, *[flat_gate(2, 3) for _ in range(5)])


EDGE_SECRETS = [0, R - 1, R, TOP, 5 * R + 7]


def tree_cases():
    cases = [_tree_case("leaf", Leaf(0), 65, EDGE_SECRETS), _tree_case("1-of-1", Threshold(1, Leaf(0)), 2, EDGE_SECRETS), _tree_case("1-of-5", flat_gate(1, 5), 65, EDGE_SECRETS)]
    for n in (2, 3, 64, 65, 256):
        cases.append(_tree_case("%d-of-%d" % (n, n), flat_gate(n, n), 2 if n > 3 else 130, EDGE_SECRETS))
        kk = n // 2 + (n > 2)
        cases.append(_tree_case("%d-of-%d" % (kk, n), flat_gate(kk, n), 2 if n > 3 else 65))
    cases += [_tree_case("1-of-1024", flat_gate(1, 1024), 2), _tree_case("1024-of-1024", flat_gate(1024, 1024), 1),
              _tree_case("example", bsw07_fixture.example_tree(), 130, EDGE_SECRETS), _tree_case("chain8", chain(8), 65, EDGE_SECRETS),
              _tree_case("16x16", sixteen_by_sixteen(), 2), _tree_case("alternating", alternating(), 65), _tree_case("3of5-2of3", three_of_five_over_two_of_three(), 1)]
    return cases


@functools.lru_cache(maxsize=None)
def _expected(label):
    c = next(c for c in tree_cases() if c["label"] == label)
    return tuple(tuple(share(c["tree"], s, q)) for s, q in zip(c["secrets"], c["coeffs"]))


def tree_expected(c):
    return [v for item in _expected(c["label"]) for v in item]


def run_tree_cases(call, cases):
    """call(node array [n, 2] uint32, secrets bytes, coeffs bytes or None, k) -> k x L scalar rows; returns the labels that differ"""
    bad = []
    for c in cases:
        flat = [v for q in c["coeffs"] for v in q]
        got = call(node_array(preorder(c["tree"])), rows(c["secrets"]), rows(flat) if flat else None, c["k"])
        if fc.ints(got) != tree_expected(c):
            bad.append(c["label"])
    return bad


MALFORMED = {
    "no nodes": [],
    "no root marker": [(0, 1), (0, 0)],
    "second root": [(ROOT_MARK, 1), (0, 0), (ROOT_MARK, 0)],
    "parent after child": [(ROOT_MARK, 1), (2, 0), (0, 1)],
    "own parent": [(ROOT_MARK, 1), (1, 0)],
    "leaf parent": [(ROOT_MARK, 1), (0, 0), (1, 0)],
    "threshold above children": [(ROOT_MARK, 3), (0, 0), (0, 0)],
    "gate without children": [(ROOT_MARK, 1), (0, 0), (0, 1)],
    "1025 children": [(ROOT_MARK, 1), (0, 1), (1, 0)] + [(0, 0)] * 1024,
    "1025 leaves": [(ROOT_MARK, 1), (0, 1)] + [(1, 0)] * 513 + [(0, 0)] * 512,
    "1025 gates": [(ROOT_MARK, 1)] + [(i, 1) for i in range(1024)] + [(1024, 0)],
}
