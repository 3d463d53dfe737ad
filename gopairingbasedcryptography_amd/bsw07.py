"""Host-side planner for batched BSW07 CP-ABE decryption (BASELINE config 4) and, below it, batched Encrypt.

The reference decrypts one ciphertext at a time by walking the threshold access tree
(access/tree/access_tree_node.go:96-164, cpabe/bsw07/bsw07_cpabe.go:172-195): per satisfied leaf two full pairings and a
GT division, per threshold node a GT.Exp by a Lagrange coefficient and a GT.Mul, then e(C, D) and two more divisions.
Mathematically

    M = C~ * A / e(C, D),      A = prod_leaves ( e(Cy, Dj) / e(Cy', Dj') ) ^ Delta_leaf

where Delta_leaf is the product of the Lagrange coefficients on the path from the leaf to the root.  Because
e(P, Q)^k = e(P, [k]Q) and 1/e(P, Q) = e(P, -Q) hold exactly as Fp12 elements, the whole decryption is ONE
multi-pairing with ONE final exponentiation per ciphertext once the exponents are folded into the key:

    Dj^ = [Delta] Dj,   Dj'^ = [-Delta] Dj'          (2 G2 scalar multiplications per used leaf, once per key and policy)
    M   = C~ * Pair([Cy..., Cy'..., -C], [Dj^..., Dj'^..., D])      (per ciphertext: 2l+1 Miller loops, 1 final exp)

This module is host orchestration only (tree walking and Lagrange coefficients in Fr, microseconds per policy); every
group operation goes through the engine (`bn254`: g2_scalar_mul, multi_pair, gt_mul).  It does not reproduce the
reference's debug pairing / prints (access_tree_node.go:99-100,116-127).
"""
import numpy as np

from . import _buffers as bufs, _plan
from ._buffers import R_ORDER


class Leaf:
    """Leaf of the access tree: satisfied when `attribute` is in the user's attribute set."""
    def __init__(self, attribute):
        self.attribute = attribute
        self.leaf_id = None


class Threshold:
    """k-of-n gate; children are numbered 1..n as in NewThresholdNode (access_tree_node.go:38-52)."""
    def __init__(self, k, *children):
        if k < 1 or k > len(children):
            raise ValueError("threshold must be between 1 and len(children)")
        self.k = k
        self.children = list(children)


def assign_leaf_ids(node, start=1):
    """Depth-first leaf numbering from 1 (GenerateLeafID, access_tree_node.go:77-94). Returns the next free id."""
    if isinstance(node, Leaf):
        node.leaf_id = start
        return start + 1
    for c in node.children:
        start = assign_leaf_ids(c, start)
    return start


def lagrange_at_zero(index, indices):
    """Delta_{index,S}(0) = prod_{j in S, j != index} (0 - j)/(index - j) mod r  (utils/compute_lagrange_basis.go:8-30)."""
    num, den = 1, 1
    for j in indices:
        if j != index:
            num = num * (-j) % R_ORDER
            den = den * (index - j) % R_ORDER
    return num * pow(den, -1, R_ORDER) % R_ORDER


def decrypt_plan(node, attributes):
    """{leaf_id: (attribute, Delta)} for the leaves the reference's DecryptNode would use (the first `k` satisfied
    children of every gate, in child order), or None when the attribute set does not satisfy the tree."""
    if isinstance(node, Leaf):
        return {node.leaf_id: (node.attribute, 1)} if node.attribute in attributes else None
    chosen = []
    for i, c in enumerate(node.children, start=1):
        sub = decrypt_plan(c, attributes)
        if sub is not None:
            chosen.append((i, sub))
            if len(chosen) == node.k:
                break
    if len(chosen) < node.k:
        return None
    idx = [i for i, _ in chosen]
    plan = {}
    for i, sub in chosen:
        d = lagrange_at_zero(i, idx)
        for leaf_id, (attr, coef) in sub.items():
            plan[leaf_id] = (attr, coef * d % R_ORDER)
    return plan


def fold_key(engine, plan, dj, dj_prime):
    """Fold the Lagrange coefficients into the user's key: rows ordered by leaf id.
    dj, dj_prime: {attribute: 128-byte G2 point}.  Returns (leaf_ids, Dj^ [l,128], Dj'^ [l,128])."""
    leaf_ids = sorted(plan)
    base = np.stack([np.asarray(dj[plan[i][0]], dtype=np.uint8) for i in leaf_ids])
    base_p = np.stack([np.asarray(dj_prime[plan[i][0]], dtype=np.uint8) for i in leaf_ids])
    pos = [plan[i][1] for i in leaf_ids]
    neg = [(-c) % R_ORDER for c in pos]
    return leaf_ids, engine.g2_scalar_mul(base, pos), engine.g2_scalar_mul(base_p, neg)


def decrypt_batch(engine, folded, d_key, cts, neg_g1):
    """Decrypt n ciphertexts under one (key, policy) plan.

    folded = fold_key(...) result; d_key = D (128 B);  cts = list of dicts with 'c_tilde' (384 B), 'c' (64 B),
    'cy' / 'cy_prime' ({leaf_id: 64 B});  neg_g1 negates an affine G1 point on the host (gnark's G1Affine.Neg).
    Returns the n messages as an [n,384] array: one fixed-Q multi-pairing call (n segments of 2l+1 pairs against the one
    folded key) and one gt_mul call."""
    leaf_ids, dj_hat, djp_hat = folded
    l = len(leaf_ids)
    Q_seg = np.concatenate([np.asarray(dj_hat).reshape(l, 128), np.asarray(djp_hat).reshape(l, 128),
                            np.asarray(d_key, dtype=np.uint8).reshape(1, 128)])
    P_rows, ctil = [], []
    for ct in cts:
        P_rows.append(np.stack([np.asarray(ct["cy"][i], dtype=np.uint8) for i in leaf_ids]
                               + [np.asarray(ct["cy_prime"][i], dtype=np.uint8) for i in leaf_ids]
                               + [neg_g1(np.asarray(ct["c"], dtype=np.uint8))]))
        ctil.append(np.asarray(ct["c_tilde"], dtype=np.uint8))
    m = 2 * l + 1
    if hasattr(engine, "multi_pair_fixed_q"):
        # the folded key is the same G2 list for every ciphertext: its Miller lines are computed once for the whole batch
        X = engine.multi_pair_fixed_q(np.concatenate(P_rows), Q_seg)
    else:
        X = engine.multi_pair(np.concatenate(P_rows), np.concatenate([Q_seg] * len(cts)), _plan.segments(len(cts), m))
    return engine.gt_mul(np.stack(ctil), X)                                          # C~ * A / e(C, D) per ciphertext


def decrypt_batch_arrays(engine, folded, d_key, c_tilde, c, cy, cy_prime):
    """The same decryption on arrays (numpy, or CUDA tensors for HBM-resident ciphertexts): n ciphertexts under one
    (key, policy) plan, BASELINE config 4 at its stated size (2^16 ciphertexts x (2 x 256 + 1) pairs).

    c_tilde [n,384], c [n,64]; cy, cy_prime [n,l,64] with the l columns in the order of folded's leaf ids.  The factor
    1 / e(C, D) enters as e(C, -D) — one host-side negation of the key's D instead of n negations of C (both equal
    e(C, D)^-1 exactly) — so the G2 list [Dj^..., Dj'^..., -D] is the same for every ciphertext: one fixed-Q multi-pairing
    (2l+1 line evaluations and one final exponentiation per ciphertext) and one gt_mul."""
    leaf_ids, dj_hat, djp_hat = folded
    l = len(leaf_ids)
    q_list = np.concatenate([np.asarray(dj_hat).reshape(l, 128), np.asarray(djp_hat).reshape(l, 128), engine.g2_neg(d_key).reshape(1, 128)])
    n = bufs.nbytes(c) // 64
    P = bufs.cat([bufs.view(cy, n, l, 64), bufs.view(cy_prime, n, l, 64), bufs.view(c, n, 1, 64)], 1)
    X = engine.multi_pair_fixed_q(bufs.flat(P), bufs.flat(bufs.put(q_list, c)))
    return engine.gt_mul(bufs.flat(c_tilde).reshape(n, 384), X)


# ------------------------------------------------------------------------------------------------ Encrypt
# cpabe/bsw07/bsw07_cpabe.go:133-170: C~ = M e(g1, g2)^(alpha s), C = h^s, and per leaf y of the policy Cy = g1^(q_y(0)), Cy' = H1(att(y))^(q_y(0)),
# the q_y(0) from AccessTreeNode.ShareSecret(s).  The sharing is engine.ShareTree (one launch for the whole batch); the randomness — s and
# the polynomial coefficients of every gate — is passed in, as in waters05.encrypt_batch and gentry06.encrypt_batch.
ROOT_MARK = 0xFFFFFFFF


def share_plan(tree):
    """(nodes, attributes) of a Leaf / Threshold tree: the node list [(parent, threshold)] in depth-first preorder that engine.ShareTree
    takes (threshold 0 = a leaf, parent ROOT_MARK for the root) and the leaves' attributes in leaf-id order.  Assigns the leaf ids as
    the reference's GenerateLeafID does (assign_leaf_ids), so column y - 1 of the shares belongs to leaf id y."""
    assign_leaf_ids(tree)
    nodes, attributes = [], []

    def walk(node, parent):
        me = len(nodes)
        if isinstance(node, Leaf):
            nodes.append((parent, 0))
            attributes.append(node.attribute)
            return
        nodes.append((parent, node.k))
        for c in node.children:
            walk(c, me)
    walk(tree, ROOT_MARK)
    return nodes, attributes


def encrypt_batch(engine, tree_or_plan, h, e_alpha, h1, messages, s, coeffs, tables=False):
    """n ciphertexts under one policy.  tree_or_plan: a Leaf / Threshold tree or share_plan(tree); h = g1^beta (64 B) and
    e_alpha = e(g1, g2)^alpha (384 B) of the public key; h1: {attribute: 64-byte G1 point} (H1 of every attribute of the policy);
    messages [n, 384]; s: n scalars; coeffs: [n, C] scalars, a gate's threshold - 1 coefficients in the order ShareSecret draws them
    (None or empty when C == 0).  Returns exactly the operands of decrypt_batch_arrays with the columns in leaf-id order:
    (c_tilde [n, 384], c [n, 64], cy [n, L, 64], cy_prime [n, L, 64]).  numpy in gives numpy out; CUDA tensors (messages, s, coeffs) give
    tensors, and only the public key, the L points of h1 and the tree go to the device.

    tables=True (opt-in; the same bytes): Cy' comes from a fixed-base table over the L points of h1 — engine.FixedBase.indexed with
    terms = 1 and the L index rows repeating per ciphertext, 32 mixed additions per leaf and no doublings — instead of the variable-base
    kernel on the L points expanded n times.  The table costs 1 MB of device memory per leaf while the call runs."""
    nodes, attributes = share_plan(tree_or_plan) if isinstance(tree_or_plan, (Leaf, Threshold)) else tree_or_plan
    L = len(attributes)
    n = bufs.nbytes(messages) // 384
    if bufs.nbytes(messages) != n * 384:
        raise ValueError("messages must hold whole GT elements")
    s = _plan.scalars(s, messages)
    coeffs = None if coeffs is None else _plan.scalars(coeffs, messages)
    bufs.device_of(messages, s, coeffs)                                              # all of one kind, on one device
    if bufs.nbytes(s) != n * 32:
        raise ValueError("s must hold n = %d scalars" % n)
    with _share_tree(engine, nodes, L) as tree:
        shares = bufs.flat(tree.share(bufs.flat(s), None if coeffs is None or not bufs.nbytes(coeffs) else bufs.flat(coeffs)))          # [n, L, 32]
    c_tilde = _plan.blind(engine, _plan.public(e_alpha, 1, 384, messages, "e_alpha"), s, messages, n)
    c = engine.g1_scalar_mul(bufs.flat(_plan.public(h, 1, 64, messages, "h")), bufs.flat(s))
    cy = engine.g1_scalar_mul_base(shares)
    hy = bufs.put(np.stack([np.asarray(h1[a], dtype=np.uint8).reshape(64) for a in attributes]), messages)
    if tables and n:
        with _plan.handle(None, lambda: engine.FixedBase(hy, g2=False), "nbase", L, "the table holds %(got)d bases for %(want)d leaves") as table:
            cy_prime, _ = table.indexed(_plan.index_rows(np.arange(L).reshape(L, 1), messages), shares, terms=1)
    else:
        cy_prime = engine.g1_scalar_mul(bufs.flat(bufs.expand(bufs.view(hy, 1, L, 64), n, L, 64)), shares)
    return bufs.view(c_tilde, n, 384), bufs.view(c, n, 64), bufs.view(cy, n, L, 64), bufs.view(cy_prime, n, L, 64)


def encrypt_batch_seeded(engine, tree_or_plan, h, e_alpha, h1, messages, rng, tables=False):
    """encrypt_batch with its randomness drawn on the device: rng is an rng.Randomness over the engine, everything else as there, and
    the return value is exactly encrypt_batch's on the scalars drawn.  The draws, in this order (the order is part of the interface:
    it is what makes the ciphertexts reproducible from the seed): s [n], then coeffs [n, C] with C the sum of (threshold - 1) over the
    gates — two stream ids, one when C == 0 (a draw of no columns takes none), none when n == 0.  The scalars are of the kind of
    `messages`: CUDA tensors in, and nothing but the seed crosses to the device.  The seed is key material: whoever holds it can
    recompute s and with it every message."""
    nodes, attributes = share_plan(tree_or_plan) if isinstance(tree_or_plan, (Leaf, Threshold)) else tree_or_plan
    n = bufs.nbytes(messages) // 384
    C = sum(int(t) - 1 for _, t in nodes if int(t))
    s = rng.scalars(messages, n)
    coeffs = rng.scalars(messages, n, C) if C else None
    return encrypt_batch(engine, (nodes, attributes), h, e_alpha, h1, messages, s, coeffs, tables=tables)


def _share_tree(engine, nodes, L):
    """engine.ShareTree over the plan's nodes, closed on the way out; its leaves must be the plan's L attributes"""
    return _plan.handle(None, lambda: engine.ShareTree(nodes), "leaves", L, "the plan names %(want)d attributes for %(got)d leaves")


# ------------------------------------------------------------------------------------------------ Decrypt, one key per item
# One policy, n users with attribute sets of their own: what decrypt_plan + fold_key do per key on the host — the walk of
# AccessTreeNode.DecryptNode and the Lagrange coefficients down every path — is engine.ShareTree.weights for the whole batch (one launch),
# and the coefficients are folded into the ciphertext's G1 components instead of the key's G2 components (half the cost; exact in Fp12
# all the same).
def leaf_mask(tree_or_plan, attribute_sets):
    """[n, L] uint8: 1 where set t holds the attribute of leaf y, the leaves in leaf-id order (column y - 1 for leaf id y) — the `held`
    of decrypt_batch_keys and of engine.ShareTree.weights.  An attribute that sits on several leaves marks all of them."""
    _, attributes = share_plan(tree_or_plan) if isinstance(tree_or_plan, (Leaf, Threshold)) else tree_or_plan
    sets = [s if isinstance(s, (set, frozenset)) else set(s) for s in attribute_sets]
    out = np.zeros((len(sets), len(attributes)), dtype=np.uint8)
    for t, s in enumerate(sets):
        out[t] = [a in s for a in attributes]
    return out


def leaf_rows(held, L):
    """nested 0 / 1 / bool values as [n][L] of 0 / 1"""
    rows = [list(h) for h in held]
    if any(len(h) != L for h in rows):
        raise ValueError("held: every item needs %d entries" % L)
    return [[1 if v else 0 for v in h] for h in rows] if rows else np.zeros((0, L), dtype=np.uint8)


def used_columns(used):
    """(index [n, U] int64, mask [n, U] uint8, U) of a [n, L] array that is non-zero where item t uses leaf y: the used columns of
    every item in ascending order, U = the largest count; the slots behind an item's last used column have mask 0 (and index 0)."""
    used = np.asarray(used) != 0
    n, L = used.shape
    count = used.sum(1)
    U = int(count.max()) if n else 0
    order = np.argsort(~used, axis=1, kind="stable")[:, :U]                          # the used columns first, each group in ascending order
    mask = (np.arange(U)[None, :] < count[:, None])
    return np.where(mask, order, 0).astype(np.int64), mask.astype(np.uint8), U


def decrypt_batch_keys(engine, tree_or_plan, held, d_key, dj, dj_prime, c_tilde, c, cy, cy_prime):
    """n (key, ciphertext) items under one policy.  tree_or_plan: a Leaf / Threshold tree or share_plan(tree); held [n, L]: non-zero
    where item t's key holds the attribute of leaf y (leaf_mask: a uint8 or bool array, nested values, or a uint8 CUDA tensor); d_key: D as [128] (one key against n ciphertexts) or [n, 128];
    dj, dj_prime [n, L, 128]: the key components of leaf y's attribute in leaf order — the rows of leaves that are not used, those
    with held = 0 among them, may hold anything: they never reach the engine, whose lists carry the all-zero encoding (the point at
    infinity) in their place; c_tilde [n, 384], c [n, 64], cy, cy_prime [n, L, 64]: the outputs of encrypt_batch, or one ciphertext
    repeated.  numpy in gives numpy out, CUDA tensors give tensors.  Returns (messages [n, 384], ok [n]): an item whose attributes do
    not satisfy the policy has ok = 0 and an all-zero row and takes no part in the group operations.

    Engine calls: ShareTree.weights (w), fr_neg (-w), one g1_scalar_mul ([w_y] Cy, [-w_y] Cy'), one multi_pair over uniform segments
    [[w] Cy ..., [-w] Cy' ..., C] against [Dj ..., Dj' ..., -D], one gt_mul with c_tilde.  Only used leaves cost Miller loops: the used
    columns of every item are gathered in leaf order up to U, the largest used count of the batch, so a segment is 2 U + 1 pairs and not
    2 L + 1; an item with fewer used leaves is padded with points at infinity, which Pair skips.  Which leaves are used comes back
    from the device once (n L bytes): the one point where the call waits for the stream."""
    nodes, attributes = share_plan(tree_or_plan) if isinstance(tree_or_plan, (Leaf, Threshold)) else tree_or_plan
    L = len(attributes)
    held, n, one_key = _keys_args(held, L, d_key, dj, dj_prime, c_tilde, c, cy, cy_prime)
    if not n:
        return bufs.zeros((0, 384), c), bufs.zeros((0,), c)
    with _share_tree(engine, nodes, L) as tree:
        w, ok = tree.weights(bufs.flat(bufs.view(held, n * L)))                      # [n, L, 32] canonical, [n]
    return _decrypt_weighted(engine, n, L, one_key, w, ok, d_key, dj, dj_prime, c_tilde, c, cy, cy_prime)


def _keys_args(held, L, d_key, dj, dj_prime, c_tilde, c, cy, cy_prime, *more):
    """(held as bytes, n, whether d_key is one key for all) of decrypt_batch_keys' arguments, checked: one kind, one device, the sizes"""
    if isinstance(held, np.ndarray):                                                 # as ShareTree.weights takes it: uint8 or bool
        if held.dtype not in (np.uint8, np.bool_):
            raise ValueError("held must be uint8 or bool (got %s)" % held.dtype)
        held = held.astype(np.uint8, copy=False)
    elif not bufs.is_torch(held):
        held = np.asarray(leaf_rows(held, L), dtype=np.uint8)
    n = bufs.nbytes(c) // 64
    one_key = bufs.nbytes(d_key) == 128                                              # a public-size value: it goes through the host like h of encrypt_batch
    bufs.device_of(held, dj, dj_prime, c_tilde, c, cy, cy_prime, *more, *([] if one_key else [d_key]))     # all of one kind, on one device
    if (bufs.nbytes(c) != n * 64 or bufs.nbytes(c_tilde) != n * 384 or bufs.nbytes(cy) != n * L * 64 or bufs.nbytes(cy_prime) != n * L * 64
            or bufs.nbytes(dj) != n * L * 128 or bufs.nbytes(dj_prime) != n * L * 128 or bufs.nbytes(held) != n * L or bufs.nbytes(d_key) not in (128, n * 128)):
        raise ValueError("need held [n, L], d_key [128] or [n, 128], dj and dj_prime [n, L, 128], c_tilde [n, 384], c [n, 64], cy and cy_prime [n, L, 64] with n = %d, L = %d" % (n, L))
    return held, n, one_key


def _decrypt_weighted(engine, n, L, one_key, w, ok, d_key, dj, dj_prime, c_tilde, c, cy, cy_prime):
    """decrypt_batch_keys behind the weights w [n, L, 32] and ok [n]: the used columns, the folding, one multi_pair, gt_mul"""
    def put(a):
        return bufs.put(a, c)

    def host(a):
        return a.cpu().numpy() if bufs.is_torch(a) else np.asarray(a)
    w = bufs.view(w, n * L, 32)
    items = _plan.Good(host(ok).reshape(n), c)
    good, ng = items.index, items.count
    if not ng:
        return items.scatter(None), bufs.view(ok, n)
    used = host(bufs.rows_nonzero(w)).reshape(n, L)[good]                            # a factor is never 0 modulo r: used <=> weight != 0
    index, mask, U = used_columns(used)
    flat_index = (good[:, None] * L + index).reshape(-1)
    keep = put(mask.reshape(-1, 1))

    def gather(a, width):
        """the used columns of the satisfied items, [ng, U, width]; the padding slots all zero"""
        return (bufs.take(bufs.view(a, n * L, width), flat_index) * keep).reshape(ng, U, width)
    wg = gather(w, 32)
    scalars = bufs.cat([wg, bufs.view(engine.fr_neg(bufs.flat(wg)), ng, U, 32)], 1)
    bases = bufs.cat([gather(cy, 64), gather(cy_prime, 64)], 1)
    folded = bufs.view(engine.g1_scalar_mul(bufs.flat(bases), bufs.flat(scalars)), ng, 2 * U, 64)
    if one_key:
        d_host = host(d_key).reshape(128)
        neg_d = bufs.expand(bufs.view(put(np.array(engine.g2_neg(d_host), dtype=np.uint8, copy=True)), 1, 1, 128), ng, 1, 128)
    else:
        d_rows = items.rows(bufs.view(d_key, n, 128))
        neg_d = bufs.view(engine.g2_sub(bufs.flat(bufs.zeros((ng, 128), c)), bufs.flat(d_rows)), ng, 1, 128)      # infinity - D
    P = bufs.cat([folded, items.rows(bufs.view(c, n, 64)).reshape(ng, 1, 64)], 1)
    Q = bufs.cat([gather(dj, 128), gather(dj_prime, 128), neg_d], 1)
    X = engine.multi_pair(bufs.flat(P), bufs.flat(Q), _plan.segments(ng, 2 * U + 1))
    msgs = engine.gt_mul(bufs.flat(items.rows(bufs.view(c_tilde, n, 384))), bufs.flat(X))
    return items.scatter(msgs), bufs.view(ok, n)


# ------------------------------------------------------------------------------------------------ a policy per ciphertext
# n items over T distinct policies: item i names its policy in policy_of[i], and engine.ShareForest walks every item's own tree in one
# launch (shares on the way in, weights on the way out).  Per-item arrays are padded to the forest's maxima: Lmax leaf columns, Cmax
# coefficient columns.  A padded column holds the all-zero encoding — a zero share, the point at infinity — and costs no group operation
# that Pair or the sums would not skip.
def forest_plan(trees):
    """(plans, attributes, index) of T Leaf / Threshold trees: plans[t] = share_plan(tree t); attributes: the distinct attributes over all
    trees in the order they are first met; index [T, Lmax] int64: the position in `attributes` of the attribute of leaf y of tree t, and
    _plan.NO_ATTRIBUTE in the columns tree t does not have."""
    plans = [share_plan(t) for t in trees]
    if not plans:
        raise ValueError("a forest needs at least one tree")
    attributes, where = [], {}
    for _, attrs in plans:
        for a in attrs:
            if a not in where:
                where[a] = len(attributes)
                attributes.append(a)
    index = np.full((len(plans), max(len(attrs) for _, attrs in plans)), _plan.NO_ATTRIBUTE, dtype=np.int64)
    for t, (_, attrs) in enumerate(plans):
        index[t, :len(attrs)] = [where[a] for a in attrs]
    return plans, attributes, index


def _forest(trees_or_plan):
    """(plans, attributes, index, Cmax) of a list of trees or of forest_plan's result"""
    is_plan = isinstance(trees_or_plan, tuple) and len(trees_or_plan) == 3 and isinstance(trees_or_plan[2], np.ndarray)
    plans, attributes, index = trees_or_plan if is_plan else forest_plan(trees_or_plan)
    return plans, attributes, index, max(sum(int(t) - 1 for _, t in nodes if int(t)) for nodes, _ in plans)


def _policy_ids(policy_of, T, like):
    """policy_of as ShareForest takes tree ids, of the kind of `like`: host values (checked against T here) as a uint32 array or, beside
    tensors, the same bits as an int32 tensor; an int32 tensor is used as it is (an id of T or more gives a zero row and ok = 0 there)"""
    if bufs.is_torch(policy_of):
        return policy_of
    ids = np.asarray(policy_of, dtype=np.int64).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() >= T):
        raise ValueError("policy_of names a policy outside 0 .. %d" % (T - 1))
    ids = ids.astype(np.uint32)
    return bufs.put(ids.view(np.int32), like) if bufs.is_torch(like) else ids


def _share_forest(engine, plans, Lmax):
    """engine.ShareForest over the plans' node lists, closed on the way out"""
    return _plan.handle(None, lambda: engine.ShareForest([nodes for nodes, _ in plans]), "leaves", Lmax, "the plans name %(want)d attributes at most for %(got)d leaves")


def encrypt_batch_policies(engine, trees_or_plan, policy_of, h, e_alpha, h1, messages, s, coeffs, tables=False):
    """n ciphertexts, ciphertext i under policy policy_of[i].  trees_or_plan: a list of T Leaf / Threshold trees or forest_plan(trees);
    policy_of: n policy numbers below T (a list, an integer array, or beside CUDA tensors an int32 tensor); h, e_alpha, messages, s as
    encrypt_batch takes them; h1: {attribute: 64-byte G1 point} for every attribute of every policy; coeffs: [n, Cmax] scalars — every
    item carries Cmax columns and uses its first C_t, gate by gate as encrypt_batch reads them; the rest may hold anything (None or empty
    when Cmax == 0).  Returns (c_tilde [n, 384], c [n, 64], cy [n, Lmax, 64], cy_prime [n, Lmax, 64]): the first L_t columns of item i
    are exactly encrypt_batch's under policy t on the same s and coefficients, and every padded column is the all-zero encoding, the
    point at infinity — what decrypt_batch_policies takes.

    Engine calls: ShareForest.share (one launch for all policies), gt_exp and gt_mul, g1_scalar_mul (C), g1_scalar_mul_base (Cy), and for
    Cy' the variable-base kernel on the H1 points gathered by policy with an all-zero row in the padding, or with tables=True (opt-in; the
    same bytes) FixedBase.indexed with terms = 1 over ONE table of the distinct H1 points, its index rows gathered by policy with
    GPBC_INDEX_NONE in the padding."""
    plans, attributes, index, Cmax = _forest(trees_or_plan)
    T, Lmax = index.shape
    n = bufs.nbytes(messages) // 384
    if bufs.nbytes(messages) != n * 384:
        raise ValueError("messages must hold whole GT elements")
    s = _plan.scalars(s, messages)
    coeffs = None if coeffs is None else _plan.scalars(coeffs, messages)
    ids = _policy_ids(policy_of, T, messages)
    bufs.device_of(messages, s, coeffs, ids)                                         # all of one kind, on one device
    if bufs.nbytes(s) != n * 32 or bufs.nbytes(ids) != n:
        raise ValueError("s and policy_of must hold n = %d entries" % n)
    if Cmax and (coeffs is None or bufs.nbytes(coeffs) != n * Cmax * 32):
        raise ValueError("coeffs must hold n x Cmax = %d x %d scalars" % (n, Cmax))
    with _share_forest(engine, plans, Lmax) as forest:
        shares, _ = forest.share(ids, bufs.flat(s), bufs.flat(coeffs) if Cmax else None)                     # [n, Lmax, 32], zero in the padding
    shares = bufs.flat(shares)
    c_tilde = _plan.blind(engine, _plan.public(e_alpha, 1, 384, messages, "e_alpha"), s, messages, n)
    c = engine.g1_scalar_mul(bufs.flat(_plan.public(h, 1, 64, messages, "h")), bufs.flat(s))
    cy = engine.g1_scalar_mul_base(shares)
    hy = np.stack([np.asarray(h1[a], dtype=np.uint8).reshape(64) for a in attributes])
    A = len(attributes)
    if tables and n:
        rows = bufs.take(_plan.index_rows(index, messages), ids)                     # [n, Lmax] of the table's kind
        with _plan.handle(None, lambda: engine.FixedBase(bufs.put(hy, messages), g2=False), "nbase", A, "the table holds %(got)d bases for %(want)d attributes") as table:
            cy_prime, _ = table.indexed(bufs.flat(rows).reshape(n * Lmax, 1), shares, terms=1)
    else:
        padded = bufs.put(np.concatenate([hy, np.zeros((1, 64), dtype=np.uint8)]), messages)                 # row A: the point at infinity
        rows = bufs.take(bufs.put(np.where(index < 0, A, index), messages), ids)
        cy_prime = engine.g1_scalar_mul(bufs.flat(bufs.take(padded, bufs.flat(rows))), shares)
    return bufs.view(c_tilde, n, 384), bufs.view(c, n, 64), bufs.view(cy, n, Lmax, 64), bufs.view(cy_prime, n, Lmax, 64)


def encrypt_batch_policies_seeded(engine, trees_or_plan, policy_of, h, e_alpha, h1, messages, rng, tables=False):
    """encrypt_batch_policies with its randomness drawn on the device: rng is an rng.Randomness over the engine, everything else as there,
    and the return value is exactly encrypt_batch_policies' on the scalars drawn.  The draws, in this order (the order is part of the
    interface: it is what makes the ciphertexts reproducible from the seed): s [n], then coeffs [n, Cmax] with Cmax the largest
    coefficient count of any policy — EVERY item draws Cmax columns, whatever its policy, and uses its first C_t.  Two stream ids, one
    when Cmax == 0 (a draw of no columns takes none), none when n == 0.  The seed is key material."""
    plan = _forest(trees_or_plan)
    n = bufs.nbytes(messages) // 384
    s = rng.scalars(messages, n)
    coeffs = rng.scalars(messages, n, plan[3]) if plan[3] else None
    return encrypt_batch_policies(engine, plan[:3], policy_of, h, e_alpha, h1, messages, s, coeffs, tables=tables)


def leaf_mask_policies(plan, policy_of, attribute_sets):
    """[n, Lmax] uint8: 1 where set i holds the attribute of leaf y of policy policy_of[i], 0 in the columns that policy does not have —
    the `held` of decrypt_batch_policies and of engine.ShareForest.weights.  plan: forest_plan(trees) or the list of trees."""
    plans, _, index, _ = _forest(plan)
    out = np.zeros((len(attribute_sets), index.shape[1]), dtype=np.uint8)
    for i, (t, held) in enumerate(zip(policy_of, attribute_sets)):
        held = held if isinstance(held, (set, frozenset)) else set(held)
        attrs = plans[int(t)][1]
        out[i, :len(attrs)] = [a in held for a in attrs]
    return out


def decrypt_batch_policies(engine, trees_or_plan, policy_of, held, d_key, dj, dj_prime, c_tilde, c, cy, cy_prime):
    """decrypt_batch_keys with a policy per item: item i is under policy policy_of[i], and every [n, L, ...] argument of decrypt_batch_keys
    is [n, Lmax, ...] here, an item's first L_t columns in its policy's leaf order — held from leaf_mask_policies, the ciphertexts from
    encrypt_batch_policies; what lies in the other columns is never used.  Returns (messages [n, 384], ok [n]): ok = 0 and an all-zero
    row where the item's attributes do not satisfy its policy (or, for ids given as a tensor, the id names no policy).  The weights come
    from ShareForest.weights, one launch for all policies; everything behind them is decrypt_batch_keys'."""
    plans, _, index, _ = _forest(trees_or_plan)
    T, Lmax = index.shape
    ids = _policy_ids(policy_of, T, c)
    held, n, one_key = _keys_args(held, Lmax, d_key, dj, dj_prime, c_tilde, c, cy, cy_prime, ids)
    if bufs.nbytes(ids) != n:
        raise ValueError("policy_of must hold n = %d entries" % n)
    if not n:
        return bufs.zeros((0, 384), c), bufs.zeros((0,), c)
    with _share_forest(engine, plans, Lmax) as forest:
        w, ok = forest.weights(ids, bufs.flat(bufs.view(held, n * Lmax)))            # [n, Lmax, 32] canonical with zero padding, [n]
    return _decrypt_weighted(engine, n, Lmax, one_key, w, ok, d_key, dj, dj_prime, c_tilde, c, cy, cy_prime)


# ------------------------------------------------------------------------------------------------ SetUp, KeyGenerate
# cpabe/bsw07/bsw07_cpabe.go:56-131.  SetUp is a handful of generator multiplications; KeyGenerate for U users over a list of A attributes
# is generator multiplications and elementwise additions except for [rj_ua] H2(a), U A variable-base multiplications in G2 with one base
# per ATTRIBUTE: the row form of g2_scalar_mul with A bases and a row of U scalars each, which from ROWS_G2_TABLE_MIN users on runs from
# a window table per attribute (csrc/rows29_g2.hip.hpp).
_host_like = _plan.like_of


def setup(engine, alpha, beta, gt_table=None):
    """(pp, msk) from the two secrets (SetUp, cpabe/bsw07/bsw07_cpabe.go:56-95).  pp = {"h": [beta] g1 (64 B), "f": [1/beta] g2 (128 B),
    "e_alpha": e(g1, g2)^alpha (384 B)} and msk = {"beta": beta (32 B), "g2_alpha": [alpha] g2 (128 B)}.  alpha, beta: a scalar each, a
    Python int, 32 bytes or a CUDA tensor (the values are of their kind).  beta = 0 gives f = the point at infinity, as the reference's
    Inverse does (0 -> 0): nothing is refused that the reference accepts.  gt_table: an engine.GTFixedBase whose base 0 is e(g1, g2),
    built once by the caller; e_alpha then comes from its indexed products and is the same bytes.  Engine calls: g1_scalar_mul_base,
    fr_inverse, g2_scalar_mul_base (1/beta and alpha in one call), pair_batch on the generators and gt_exp (or gt_table.indexed, one
    term)."""
    like = _host_like(alpha, beta)
    alpha, beta = _plan.scalars(alpha, like, 1, "alpha"), _plan.scalars(beta, like, 1, "beta")
    bufs.device_of(alpha, beta)
    g2s = bufs.view(engine.g2_scalar_mul_base(bufs.flat(bufs.cat([bufs.view(engine.fr_inverse(beta), 1, 32), bufs.view(alpha, 1, 32)]))), 2, 128)
    if gt_table is None:
        g1, g2 = engine.generators()
        e = _plan.public(np.asarray(engine.pair_batch(np.asarray(g1, dtype=np.uint8).reshape(-1), np.asarray(g2, dtype=np.uint8).reshape(-1))), 1, 384, like, "e")
        e_alpha = engine.gt_exp(bufs.flat(e), alpha)
    else:
        e_alpha, _ = gt_table.indexed(_plan.index_rows(np.array([[0]]), like), alpha, terms=1)
    pp = {"h": bufs.view(engine.g1_scalar_mul_base(beta), 64), "f": g2s[0], "e_alpha": bufs.view(e_alpha, 384)}
    return pp, {"beta": bufs.view(beta, 32), "g2_alpha": g2s[1]}


def setup_seeded(engine, rng, like=None, gt_table=None):
    """setup with the secrets drawn on the device: rng is an rng.Randomness over the engine.  The draws, in this order (the order is part
    of the interface: it is what makes the keys reproducible from the seed): alpha, then beta — two stream ids.  like: a buffer of the
    kind the keys are to be (None: host arrays).  The seed is key material: whoever holds it holds the master secret key."""
    like = np.zeros(0, dtype=np.uint8) if like is None else like
    alpha = rng.scalars(like, 1)
    beta = rng.scalars(like, 1)
    return setup(engine, alpha, beta, gt_table=gt_table)


def keygen_batch(engine, msk, h2, r, rj, held=None):
    """The keys of U users over a list of A attributes (KeyGenerate, cpabe/bsw07/bsw07_cpabe.go:97-131): (D [U, 128], dj [U, A, 128],
    dj_prime [U, A, 128]) with D_u = [1/beta]([alpha] g2 + [r_u] g2), dj[u, a] = [r_u] g2 + [rj_ua] H2(a), dj_prime[u, a] = [rj_ua] g2.
    msk: setup's; h2 [A, 128]: H2 of the A attributes; r: U scalars; rj [U, A] scalars, user-major as the reference draws them (Python
    ints, uint8 arrays or CUDA tensors; numpy in gives numpy out, tensors give tensors).  held [U, A] bytes: non-zero = user u gets
    attribute a; the other rows of dj and dj_prime come out all zero (None: every attribute to every user).

    h2=None reproduces the reference, whose Hash2BSw07 returns the generator for every attribute: dj = [r + rj] g2 by fr_add and one
    generator multiplication — the bytes the row route gives with h2 = the generator repeated.

    Engine calls: g2_scalar_mul_base (R = [r] g2), g2_add with g2_alpha and g2_scalar_mul by fr_inverse(beta) with a base per scalar (D),
    g2_scalar_mul_base (dj_prime), ONE g2_scalar_mul in its row form — A bases, A U scalars, rj permuted to attribute-major: one base
    per attribute and a row of U scalars per base — and g2_add of its result permuted back with R expanded over A (dj)."""
    like = _host_like(r, rj, h2)
    r, rj = _plan.scalars(r, like), _plan.scalars(rj, like)
    U = bufs.nbytes(r) // 32
    if bufs.nbytes(r) != U * 32:
        raise ValueError("r must hold whole 32-byte scalars")
    if h2 is None:
        A = bufs.nbytes(rj) // (32 * U) if U else 0
    else:
        A = bufs.nbytes(h2) // 128
        if bufs.nbytes(h2) != A * 128:
            raise ValueError("h2 must hold whole G2 points")
        h2 = _plan.public(h2, A, 128, like, "h2")
    if bufs.nbytes(rj) != U * A * 32:
        raise ValueError("rj must hold U x A = %d x %d scalars" % (U, A))
    bufs.device_of(r, rj, *([] if h2 is None else [h2]))
    if held is not None:
        held = _plan.public(held, U * A, 1, like, "held")
    g2_alpha = _plan.public(msk["g2_alpha"], 1, 128, like, "msk g2_alpha")
    beta = bufs.flat(_plan.public(msk["beta"], 1, 32, like, "msk beta"))
    if not U:
        return bufs.zeros((0, 128), like), bufs.zeros((0, A, 128), like), bufs.zeros((0, A, 128), like)
    R = bufs.view(engine.g2_scalar_mul_base(bufs.flat(r)), U, 128)
    inv = bufs.view(engine.fr_inverse(beta), 1, 32)
    D = engine.g2_scalar_mul(engine.g2_add(bufs.flat(R), bufs.flat(bufs.expand(g2_alpha, U, 128))), bufs.flat(bufs.expand(inv, U, 32)))
    if not A:
        return bufs.view(D, U, 128), bufs.zeros((U, 0, 128), like), bufs.zeros((U, 0, 128), like)
    rj = bufs.view(rj, U, A, 32)
    dj_prime = bufs.view(engine.g2_scalar_mul_base(bufs.flat(rj)), U * A, 128)
    if h2 is None:
        dj = engine.g2_scalar_mul_base(engine.fr_add(bufs.flat(bufs.expand(bufs.view(r, U, 1, 32), U, A, 32)), bufs.flat(rj)))
    else:
        T = bufs.view(engine.g2_scalar_mul(bufs.flat(h2), bufs.flat(rj.swapaxes(0, 1))), A, U, 128)
        dj = engine.g2_add(bufs.flat(T.swapaxes(0, 1)), bufs.flat(bufs.expand(bufs.view(R, U, 1, 128), U, A, 128)))
    dj = bufs.view(dj, U * A, 128)
    if held is not None:
        keep = bufs.view(bufs.rows_nonzero(held), U * A, 1)
        dj, dj_prime = dj * keep, dj_prime * keep
    return bufs.view(D, U, 128), bufs.view(dj, U, A, 128), bufs.view(dj_prime, U, A, 128)


def keygen_batch_seeded(engine, msk, h2, n_users, rng, n_attrs=None, held=None, like=None):
    """keygen_batch with its randomness drawn on the device: rng is an rng.Randomness over the engine, everything else as there, and the
    return value is exactly keygen_batch's on the scalars drawn.  The draws, in this order (the order is part of the interface: it is
    what makes the keys reproducible from the seed): r [U], then rj [U, A] — two stream ids, one when A == 0, none when U == 0.  A is
    h2's, or n_attrs with h2=None.  like: a buffer of the kind the keys are to be (None: h2's kind, host arrays without it).  The seed
    is key material: whoever holds it can recompute every user's r."""
    like = _host_like(h2) if like is None else like
    A = int(n_attrs) if h2 is None else bufs.nbytes(h2) // 128
    r = rng.scalars(like, int(n_users))
    rj = rng.scalars(like, int(n_users), A)
    return keygen_batch(engine, msk, h2, r, rj, held=held)


def key_for_leaves(tree_or_plan, attrs, held, dj, dj_prime):
    """keygen_batch's keys over the attribute list `attrs` as decrypt_batch_keys takes them: (held [U, L], dj [U, L, 128],
    dj_prime [U, L, 128]) with the columns in leaf order.  tree_or_plan: a Leaf / Threshold tree or share_plan(tree); attrs: the A
    attributes of the columns of dj and dj_prime [U, A, 128]; held [U, A] as keygen_batch took it (None: every attribute to every user).
    An attribute that sits on several leaves goes to all of them; a leaf whose attribute is not in attrs has held = 0 and zero rows."""
    _, attributes = share_plan(tree_or_plan) if isinstance(tree_or_plan, (Leaf, Threshold)) else tree_or_plan
    attrs = list(attrs)
    A, L = len(attrs), len(attributes)
    if len(set(attrs)) != A:
        raise ValueError("attrs names an attribute twice")
    U = bufs.nbytes(dj) // (128 * A) if A else 0
    if not A or bufs.nbytes(dj) != U * A * 128 or bufs.nbytes(dj_prime) != U * A * 128:
        raise ValueError("need dj and dj_prime [U, A, 128] over A = %d >= 1 attributes" % A)
    bufs.device_of(dj, dj_prime)
    where = {a: i for i, a in enumerate(attrs)}
    column = np.array([where.get(a, A) for a in attributes], dtype=np.int64)         # column A: the padding, all zero
    held = bufs.zeros((U, A), dj) + 1 if held is None else bufs.view(bufs.rows_nonzero(_plan.public(held, U * A, 1, dj, "held")), U, A)

    def leaves(a, width):
        padded = bufs.cat([bufs.view(a, U, A, width), bufs.zeros((U, 1, width), dj)], 1)
        return bufs.take(padded, column, axis=1)
    h = leaves(held, 1)
    return bufs.view(h, U, L), leaves(dj, 128) * h, leaves(dj_prime, 128) * h
