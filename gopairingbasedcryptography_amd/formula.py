"""Boolean formulas as LSSS policies: what the reference's users write with And / Or / Leaf (access/lsss/binary_access_tree_utils.go) and
NewLSSSMatrixFromBinaryTree (access/lsss/lewko_waters_lsss_matrix.go:34-87) turns into the Lewko-Waters share matrix.

A formula is a nested tuple — ("and", l, r), ("or", l, r), or an integer leaf, its attribute in [0, 2^63) — and, encoded, a row of int64
codes: the nodes of the tree in depth-first preorder (gate, left subtree, right subtree), a code >= 0 a leaf, AND and OR the gates, END
the padding behind the tree (include/gpbc_bn254_formula.h).  A row is well formed when, starting from need = 1, every node takes 1 and a
gate adds 2, the tree ends where need reaches 0, only END follows, and no END or code below OR comes before.

encode makes the rows; check, leaves and size read them in vectorised numpy (no loop over the items: the loops below run over the at
most 127 node positions).  lsss_matrix is the builder for one formula in Python integers, for the one-policy planners (lw11.py).  padded
makes the waters11.Padded block of a batch with the matrix built by engine.fr_lsss_from_formula, in HBM when the batch lives there.

Host-side and engine-agnostic like the planners: an engine is only ever an argument."""
import numpy as np

from . import _buffers as bufs
from ._buffers import R_ORDER

AND, OR, END = -2, -3, -1
MAX_NODES, MAX_LEAVES = 127, 64
_GATES = {"and": AND, "or": OR}


def _codes(f, out):
    """the preorder codes of one nested formula, appended to `out` (iterative: a formula may be 64 gates deep)"""
    todo = [f]
    while todo:
        node = todo.pop()
        if isinstance(node, (int, np.integer)) and not isinstance(node, bool):
            if not 0 <= int(node) < 1 << 63:
                raise ValueError("attributes must be integers in [0, 2^63) (got %d)" % int(node))
            out.append(int(node))
        elif isinstance(node, (tuple, list)) and len(node) == 3 and isinstance(node[0], str) and node[0].lower() in _GATES:
            out.append(_GATES[node[0].lower()])
            todo += [node[2], node[1]]
        else:
            raise ValueError("a formula is an integer leaf, ('and', l, r) or ('or', l, r) (got %r)" % (node,))
        if len(out) > MAX_NODES:
            raise ValueError("a formula holds at most %d nodes (%d leaves)" % (MAX_NODES, MAX_LEAVES))
    return out


def encode(formulas, n_nodes=None):
    """nested formulas -> [n, N] int64 codes, N the largest node count (or n_nodes), END behind each tree.  A formula object that
    occurs again is encoded once."""
    formulas = list(formulas)                     # every object stays alive while its id is a key (a generator's tuples would not)
    done, rows = {}, []
    for f in formulas:
        key = id(f) if isinstance(f, (tuple, list)) else ("leaf", f)
        if key not in done:
            done[key] = _codes(f, [])
        rows.append(done[key])
    N = max([len(r) for r in rows] + [1]) if n_nodes is None else int(n_nodes)
    if not 1 <= N <= MAX_NODES or any(len(r) > N for r in rows):
        raise ValueError("n_nodes must be in 1 .. %d and hold the largest formula (%d nodes)" % (MAX_NODES, max([len(r) for r in rows] + [1])))
    out = np.full((len(rows), N), END, dtype=np.int64)
    for t, r in enumerate(rows):
        out[t, :len(r)] = r
    return out


def _rows(nodes):
    nodes = np.asarray(nodes.cpu() if bufs.is_torch(nodes) else nodes)
    if nodes.dtype != np.int64 or nodes.ndim not in (1, 2) or not 1 <= nodes.shape[-1] <= MAX_NODES:
        raise ValueError("nodes must be int64 codes [n, N] or [N], N in 1 .. %d" % MAX_NODES)
    return nodes.reshape(-1, nodes.shape[-1])


def _shape(nodes):
    """(ok [n] bool, inside [n, N] bool: the node belongs to the tree) by the rule of the module docstring"""
    nodes = _rows(nodes)
    step = np.where(nodes >= 0, -1, np.where((nodes == AND) | (nodes == OR), 1, 0))
    need = 1 + np.cumsum(step, axis=1)                                         # after each node, as if the tree never ended
    ended = np.cumsum(need == 0, axis=1) > 0                                   # at or behind the first node where need reaches 0
    inside = np.concatenate([np.ones((len(nodes), 1), dtype=bool), ~ended[:, :-1]], axis=1)
    legal = np.where(inside, (nodes >= 0) | (nodes == AND) | (nodes == OR), nodes == END)
    return legal.all(1) & ended[:, -1], inside


def check(nodes):
    """[n] uint8: 1 where the row is a well-formed formula"""
    return _shape(nodes)[0].astype(np.uint8)


def leaves(nodes, rows=None, strict=True):
    """[n, R] int64: the attributes of each formula's leaves in order, NO_ATTRIBUTE (-1) behind them — the rho table of the matrices of
    fr_lsss_from_formula.  R = the largest leaf count, or `rows`.  Every row must be well formed and fit; with strict=False a row that
    is not is all NO_ATTRIBUTE, as the device entries leave it (ok = 0)."""
    nodes = _rows(nodes)
    ok, inside = _shape(nodes)
    if strict and not ok.all():
        raise ValueError("formula %d is malformed" % int(np.nonzero(~ok)[0][0]))
    leaf = inside & (nodes >= 0) & ok[:, None]
    count = leaf.sum(1)
    R = max(int(count.max()) if len(nodes) else 1, 1) if rows is None else int(rows)
    if strict and len(nodes) and int(count.max()) > R:
        raise ValueError("formula %d has %d leaves, more than the %d rows" % (int(count.argmax()), int(count.max()), R))
    leaf &= (count <= R)[:, None]
    table = np.full((len(nodes), R), END, dtype=np.int64)
    t, u = np.nonzero(leaf)
    table[t, (np.cumsum(leaf, axis=1) - 1)[t, u]] = nodes[t, u]
    return table


def size(nodes):
    """(rows, cols): the largest leaf count and the largest column count (1 + the number of AND gates) over well-formed rows"""
    nodes = _rows(nodes)
    ok, inside = _shape(nodes)
    if not ok.all():
        raise ValueError("formula %d is malformed" % int(np.nonzero(~ok)[0][0]))
    if not len(nodes):
        return 1, 1
    return int((inside & (nodes >= 0)).sum(1).max()), 1 + int((inside & (nodes == AND)).sum(1).max())


def lsss_matrix(formula):
    """(matrix, rho) of one formula in Python integers, as lw11.encrypt_batch and lw11.reconstruction_weights take them:
    NewLSSSMatrixFromBinaryTree.  formula: a nested formula or one row of codes.  -1 is r - 1."""
    if isinstance(formula, np.ndarray) or bufs.is_torch(formula):
        codes = _rows(formula)
        if len(codes) != 1 or not check(codes)[0]:
            raise ValueError("need one well-formed row of codes")
        codes = [int(c) for c in codes[0] if c != END]
    else:
        codes = _codes(formula, [])
    vector, counter, pending, matrix, rho = [1], 1, [], [], []
    for c in codes:
        if c >= 0:
            matrix.append(vector)
            rho.append(c)
            vector = pending.pop() if pending else None
        elif c == OR:
            pending.append(list(vector))
        else:
            pending.append(vector + [0] * (counter - len(vector)) + [1])
            vector = [0] * counter + [R_ORDER - 1]
            counter += 1
    return [row + [0] * (counter - len(row)) for row in matrix], rho


def padded(engine, nodes, like=None, rows=None, cols=None):
    """The waters11.Padded block of a batch of formulas: the matrix [n, R, C, 32] from engine.fr_lsss_from_formula — a device buffer
    when `like` is a tensor, and then it never was on the host — and rho [n, R], the host table the planners index with.  R, C: the
    largest row and column counts, or the ones given.  A malformed or oversized formula is a ValueError before the engine is touched."""
    from .waters11 import Padded
    table = _rows(nodes)
    need_r, need_c = size(table)
    R, C = need_r if rows is None else int(rows), need_c if cols is None else int(cols)
    if not 1 <= R <= MAX_LEAVES or not 1 <= C <= MAX_LEAVES or need_r > R or need_c > C:
        raise ValueError("the formulas need %d rows and %d columns, [%s, %s] in 1 .. %d do not hold them" % (need_r, need_c, R, C, MAX_LEAVES))
    rho = leaves(table, R)
    if like is not None and bufs.is_torch(like):
        dev_nodes = nodes if bufs.is_torch(nodes) and nodes.device == like.device else bufs.put(np.ascontiguousarray(table), like)
    else:
        dev_nodes = np.ascontiguousarray(table)
    matrix = engine.fr_lsss_from_formula(dev_nodes.reshape(len(table), table.shape[1]), R, C)[0]
    return Padded(matrix, rho, R, C)
