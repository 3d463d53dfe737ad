"""Inputs and expectations of the threshold-tree forest tests (tests/test_fr_forest.py on the CPU harness, tests/test_fr_forest_gpu.py on
the device): forests built from the trees tests/share_cases.py and tests/tree_weight_cases.py already have, so that one call mixes a
single leaf, 2-of-3, the example tree, chain8 (the deepest), 65-of-65 (a level wider than a wave), 16x16 (E = 272, the edge of the small
LDS instance), many-gates (a second forest, the large instance) and the largest tree a handle accepts (one item).  tree_of interleaves the
trees; the per-item arrays are padded to the forest's maxima with garbage where the kernels must not look (coefficients beyond C_t, held
bytes beyond L_t).  Expectations are Python integers per item and nothing else: an item's secret, coefficients and shares are those of its
tree's own case in share_cases (tree_expected), its held row and weights those of tree_weight_cases (bsw07.decrypt_plan), the padded
columns zero, and an item whose tree id is out of range an all-zero row with ok = 0.  Every comparison is exact."""
import numpy as np

import fr_cases as fc
import share_cases as sc
import tree_weight_cases as tw

R = fc.R
GARBAGE = (0xFF, 0x01, 0x80)                     # what lies in the padded columns of held, and fills the padded coefficients
BAD_IDS = ("T", 0xFFFFFFFF)                      # an item with one of these names no tree: T itself, and the largest id

FORESTS = {
    "mixed": ("leaf", "2-of-3", "example", "chain8", "65-of-65"),
    "edge": ("16x16", "leaf", "chain8", "2-of-3", "example", "65-of-65"),
    "large": ("many-gates", "leaf", "2-of-3"),
    "largest": ("leaf", "largest"),
}


_TREES = {}


def tree(label):
    """{tree (leaf y = attribute y), L, C, nodes, secrets, coeffs, shares: per variant; held, weights, ok: per variant} of one tree, built
    once: the variants are the items of the tree's own cases in the two case modules"""
    if label in _TREES:
        return _TREES[label]
    t, L = next((t, L) for name, t, L in tw.trees() if name == label)
    C = sc.n_coeffs(t)
    shared = next((c for c in sc.tree_cases() if c["label"] == label), None)
    if shared is not None:
        secrets, coeffs = shared["secrets"], shared["coeffs"]
        flat = sc.tree_expected(shared)
        shares = [flat[j * L:(j + 1) * L] for j in range(shared["k"])]
    else:                                           # many-gates, largest: not in share_cases; one sharing, restated here
        secrets, coeffs = sc.rand("forest-s-" + label, 1), [sc.rand("forest-q-" + label, C)]
        shares = [sc.share(t, secrets[0], coeffs[0])]
    held = [row for c in tw.cases() if c["label"].split("/")[0] == label for row in c["held"]]
    rows = [tw.expected_row(label, t, L, m) for m in held]
    _TREES[label] = dict(tree=t, L=L, C=C, nodes=sc.preorder(t), secrets=secrets, coeffs=coeffs, shares=shares, held=held, weights=[r for r, _ in rows], ok=[o for _, o in rows])
    return _TREES[label]


def forest_nodes(labels):
    """(nodes [n, 2] uint32, node_off [T + 1] uint32) of the trees' node lists one behind the other"""
    lists = [tree(l)["nodes"] for l in labels]
    off = np.cumsum([0] + [len(n) for n in lists]).astype(np.uint32)
    return sc.node_array([n for lst in lists for n in lst]), off


def _case(label, forest, tree_of):
    labels = FORESTS[forest]
    T, trees = len(labels), [tree(l) for l in labels]
    Lmax, Cmax = max(t["L"] for t in trees), max(t["C"] for t in trees)
    k = len(tree_of)
    ids = np.array([T if t == "T" else t for t in tree_of], dtype=np.uint32)
    nodes, node_off = forest_nodes(labels)
    secrets, coeffs = [], np.zeros((k, max(Cmax, 1), 32), dtype=np.uint8)
    held = np.zeros((k, Lmax), dtype=np.uint8)
    want_s, want_w, want_ok, want_valid = [], [], [], []
    seen = [0] * T
    for i, t in enumerate(ids):
        coeffs[i] = GARBAGE[i % 3]                   # everything an item's tree does not own stays this
        held[i] = GARBAGE[(i + 1) % 3]
        if t >= T:
            secrets.append(sc.rand("forest-bad-" + label, i + 1)[i])
            want_s += [0] * Lmax
            want_w += [0] * Lmax
            want_ok.append(0)
            want_valid.append(0)
            continue
        tr, j = trees[t], seen[t]
        seen[t] += 1
        js, jh = j % len(tr["secrets"]), j % len(tr["held"])
        secrets.append(tr["secrets"][js])
        if tr["C"]:
            coeffs[i, :tr["C"]] = fc.rows(tr["coeffs"][js])
        held[i, :tr["L"]] = tr["held"][jh]
        want_s += list(tr["shares"][js]) + [0] * (Lmax - tr["L"])
        want_w += list(tr["weights"][jh]) + [0] * (Lmax - tr["L"])
        want_ok.append(tr["ok"][jh])
        want_valid.append(1)
    return dict(label=label, forest=forest, labels=labels, T=T, k=k, Lmax=Lmax, Cmax=Cmax, L=[t["L"] for t in trees], C=[t["C"] for t in trees], nodes=nodes, node_off=node_off,
                tree_of=ids, secrets=fc.rows(secrets), coeffs=coeffs[:, :Cmax], held=held, want_shares=want_s, want_valid=want_valid, want_w=want_w, want_ok=want_ok)


def interleaved(T, k, shift=0):
    """tree ids in turn, so that neighbours — the items of one workgroup — belong to different trees"""
    return [(i + shift) % T for i in range(k)]


_CASES = []


def cases():
    """the case list, built once (callers leave it as it is)"""
    if not _CASES:
        _CASES.extend(_build_cases())
    return _CASES


def _build_cases():
    """Item counts 1, 3, 65 and 130.  mixed at 130 is three workgroups and more at either kernel; bad-ids carries T and 0xffffffff among
    valid items, at the front of a workgroup and at the very end.  The heavy trees come seldom: 16x16 every sixth item, many-gates every
    third of 11, the largest tree once."""
    out = [_case("mixed/%d" % k, "mixed", interleaved(5, k, shift=k)) for k in (1, 3, 65, 130)]
    bad = interleaved(5, 65)
    bad[0], bad[17], bad[40], bad[64] = "T", 0xFFFFFFFF, "T", 0xFFFFFFFF
    out.append(_case("mixed/bad-ids", "mixed", bad))
    out.append(_case("edge/65", "edge", interleaved(6, 65)))
    out.append(_case("large/11", "large", interleaved(3, 11)))
    out.append(_case("largest/1", "largest", [1]))
    return out


def run_share(call, cases_):
    """call(case) -> (k x Lmax scalar rows, k ok bytes); returns the labels that differ"""
    bad = []
    for c in cases_:
        out, ok = call(c)
        if fc.ints(out) != c["want_shares"] or [int(v) for v in np.asarray(ok).reshape(-1)] != c["want_valid"]:
            bad.append(c["label"])
    return bad


def run_weights(call, cases_):
    """call(case) -> (k x Lmax scalar rows, k ok bytes); returns the labels that differ"""
    bad = []
    for c in cases_:
        w, ok = call(c)
        if fc.ints(w) != c["want_w"] or [int(v) for v in np.asarray(ok).reshape(-1)] != c["want_ok"]:
            bad.append(c["label"])
    return bad
