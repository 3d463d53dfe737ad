"""Host-side planner for batched Sahai-Waters 2005 fuzzy identity-based decryption (fibe/sw05_fibe_common.go:284-333 and
fibe/sw05_fibe_large_universe.go:244-291): one user key against a batch of ciphertexts, computeT (sw05_fibe_large_universe.go:
302-325) for many attributes at once, and KeyGenerate of both universes for many users at once (keygen_batch, keygen_batch_large below).

What is computed.  Per ciphertext, S = FindCommonAttributes(S_user, S_msg, d) (utils/find_common_attributes.go: the first d distinct
attributes of the CIPHERTEXT's list that the key holds) and Delta_i = ComputeLagrangeBasis(i, S, 0) for i in S, then

    small universe   M = e' / prod_i e(D_i, E_i)^Delta_i                  = e' / Pair([Delta_i] D_i ..., E_i ...)
    large universe   M = e' * prod_i (e(d_i, E_i) / e(E'', D_i))^Delta_i  = e' * Pair([Delta_i] d_i ..., [-Delta_i] E'' ...; E_i ..., D_i ...)

The exponent folds in front of the pairing exactly — e(P, Q)^k = e([k] P, Q) as Fp12 elements, the argument lw11.py makes for its
weights — so a ciphertext costs one multi-pairing segment (one final exponentiation) and no GT exponentiation.  S differs from
ciphertext to ciphertext, so unlike the coefficients of bsw07.py and lw11.py (one policy for the whole batch, host integers) the
Delta_i are per item: engine.fr_lagrange_basis makes them on the device, n rows of d at a time, and they go into
engine.g1_scalar_mul as they are.

Host orchestration only, engine-agnostic (every function takes the engine: `bn254`, or a stand-in with the same function names).
Host arrays in give host arrays out; CUDA tensors in give CUDA tensors out, with only the key, the selected attribute values and
index tables going to the device.  Every ciphertext of a batch carries the same number of attributes.

Two input forms.  Attributes as nested Python integers: the selection is select_common below, a host loop per ciphertext.  Attributes as
scalar rows ([n, a, 32] uint8, an array or a CUDA tensor — where hash_to_field, sha256(to_fr=True) or an unmarshalled ciphertext left
them): the selection is engine.fr_find_common, its `common` rows are the Lagrange sets as they are, the gathers take its positions on the
device, and only ok (n bytes) comes back to the host — the call's one wait.  Both forms give the same bytes."""
import numpy as np

from . import _buffers as bufs, _plan
from ._buffers import R_ORDER


def attribute_rows(values):
    """attribute values (Python ints, reduced modulo r) as scalar rows: [len, 32] uint8, or [n, a, 32] for nested lists [n][a] of one
    length — what the rows form of decrypt_batch / decrypt_batch_large and engine.fr_find_common take"""
    values = list(values)
    if values and isinstance(values[0], (list, tuple)):
        a = len(values[0])
        if any(len(v) != a for v in values):
            raise ValueError("every row needs %d values" % a)
        return _plan.scalar_rows(values).reshape(len(values), a, 32)
    return _plan.scalar_rows(values)


def _is_rows(x):
    return _plan.is_buffer(x) and len(x.shape) == 3 and x.shape[2] == 32 and str(x.dtype) in ("uint8", "torch.uint8")


def select_common(key_attrs, ct_attrs, d):
    """FindCommonAttributes(S_user, S_msg, d) for every ciphertext: walk the ciphertext's list in order and keep the first d distinct
    attributes (as field elements: modulo r) that the key holds.  Returns (key_pos [n, d], ct_pos [n, d], ok [n]): the positions of
    the kept attributes in the key's list (its first occurrence) and in the ciphertext's list; ok = 0, and positions 0, where fewer
    than d are common (the reference returns nil and Decrypt fails)."""
    if d < 1:
        raise ValueError("d must be at least 1 (got %s)" % d)
    first = {}
    for p, a in enumerate(key_attrs):
        first.setdefault(int(a) % R_ORDER, p)
    n = len(ct_attrs)
    key_pos, ct_pos, ok = np.zeros((n, d), dtype=np.int64), np.zeros((n, d), dtype=np.int64), np.zeros(n, dtype=np.uint8)
    get = first.get
    for t, attrs in enumerate(ct_attrs):
        seen, kp, cp = set(), [], []
        for p, a in enumerate(attrs):
            pos = get(a)
            if pos is None:                                         # not there as it is written; as a field element?
                a = int(a) % R_ORDER
                pos = get(a)
                if pos is None:
                    continue
            else:
                a = int(a) % R_ORDER
            if a not in seen:
                seen.add(a)
                kp.append(pos)
                cp.append(p)
                if len(kp) == d:
                    break
        if len(kp) == d:
            key_pos[t], ct_pos[t], ok[t] = kp, cp, 1
    return key_pos, ct_pos, ok


class _Plan:
    """what both decrypts share: the selection, the Lagrange coefficients of the decryptable ciphertexts and the gathers"""

    def __init__(self, engine, key_attrs, d, ct_attrs, E, e_prime):
        self.engine, self.d, self.n = engine, d, len(ct_attrs)
        bufs.device_of(E, e_prime)                                              # both of one kind, on one device
        a = len(ct_attrs[0]) if self.n else 0
        if any(len(c) != a for c in ct_attrs):
            raise ValueError("every ciphertext of a batch needs the same number of attributes")
        if bufs.nbytes(E) != self.n * a * 128 or bufs.nbytes(e_prime) != self.n * 384:
            raise ValueError("E must hold n x %d G2 points and e_prime n GT elements (n = %d)" % (a, self.n))
        self.E, self.e_prime = bufs.view(E, self.n, a, 128), bufs.view(e_prime, self.n, 384)
        self.key_pos, self.ct_pos, ok = select_common(key_attrs, ct_attrs, d)
        if not self._select(ok):
            return
        pos = self.ct_pos.tolist()
        sets = _plan.scalar_rows(ct_attrs[t][p] for t in self.good.tolist() for p in pos[t])
        self.delta = engine.fr_lagrange_basis(self.put(sets).reshape(-1), d).reshape(self.ng * d, 32)      # x = 0, the nodes are the set

    def _select(self, ok):
        """the decryptable ciphertexts from the host's ok; their count"""
        self.ok, self.items = ok, _plan.Good(ok, self.E)
        self.good, self.ng, self.rows = self.items.index, self.items.count, self.items.rows
        return self.ng

    def put(self, a):
        return bufs.put(a, self.E)

    def seg(self, pairs):
        return _plan.segments(self.ng, pairs)

    def key_rows(self, comp, width):
        """the key component at the selected positions: [ng, d, width]"""
        return self.put(np.asarray(comp, dtype=np.uint8).reshape(-1, width)[self.key_pos[self.good].reshape(-1)]).reshape(self.ng, self.d, width)

    def ct_rows(self):
        """E_i of the selected attributes: [ng, d, 128]"""
        index = (self.good[:, None] * self.E.shape[1] + self.ct_pos[self.good]).reshape(-1)
        return bufs.take(self.E.reshape(-1, 128), index).reshape(self.ng, self.d, 128)

    def scatter(self, msgs):
        """messages of the decryptable ciphertexts into n rows; the others stay all zero"""
        return self.items.scatter(msgs), self.put(self.ok.copy())


class _RowsPlan(_Plan):
    """the same from attribute rows: the selection on the device, its positions used where they are"""

    def __init__(self, engine, key_attrs, d, ct_attrs, E, e_prime):
        if d < 1:
            raise ValueError("d must be at least 1 (got %s)" % d)
        self.engine, self.d, self.n = engine, d, int(ct_attrs.shape[0])
        n, a = self.n, int(ct_attrs.shape[1])
        if not _plan.is_buffer(key_attrs):
            key_attrs = bufs.put(attribute_rows(key_attrs), ct_attrs)                         # converted once
        shape = tuple(key_attrs.shape)
        if len(shape) not in (2, 3) or shape[-1] != 32 or (len(shape) == 3 and shape[0] != n):
            raise ValueError("the key's attributes must be [m, 32] or [n, m, 32] scalar rows (n = %d)" % n)
        bufs.device_of(ct_attrs, key_attrs, E, e_prime)                                       # all of one kind, on one device
        self.per_item, self.m, self.a = len(shape) == 3, int(shape[-2]), a
        if bufs.nbytes(E) != n * a * 128 or bufs.nbytes(e_prime) != n * 384:
            raise ValueError("E must hold n x %d G2 points and e_prime n GT elements (n = %d)" % (a, n))
        self.E, self.e_prime = bufs.view(E, n, a, 128), bufs.view(e_prime, n, 384)
        if not n:
            self._select(np.zeros(0, dtype=np.uint8))
            return
        set_pos, list_pos, common, ok = engine.fr_find_common(bufs.flat(key_attrs), bufs.flat(ct_attrs), self.m, a, d)
        ng = self._select(np.array(ok.cpu().numpy() if bufs.is_torch(ok) else ok, dtype=np.uint8, copy=True).reshape(n))      # the one wait
        if not ng:
            return
        self.key_pos, self.ct_pos = bufs.take(set_pos.reshape(n, d), self.good), bufs.take(list_pos.reshape(n, d), self.good)
        self.delta = engine.fr_lagrange_basis(bufs.flat(bufs.take(common.reshape(n, d * 32), self.good)), d).reshape(ng * d, 32)

    def _index(self, pos, width):
        """positions inside the rows of the decryptable items as positions in the flattened [n x width] table"""
        return (pos + self.put(self.good * width).reshape(self.ng, 1)).reshape(-1)

    def key_rows(self, comp, width):
        comp = comp if bufs.is_torch(comp) else self.put(np.asarray(comp, dtype=np.uint8))
        if bufs.nbytes(comp) != (self.n if self.per_item else 1) * self.m * width:
            raise ValueError("a key component must hold %s%d x %d bytes" % ("n x " if self.per_item else "", self.m, width))
        index = self._index(self.key_pos, self.m) if self.per_item else self.key_pos.reshape(-1)
        return bufs.take(comp.reshape(-1, width), index).reshape(self.ng, self.d, width)

    def ct_rows(self):
        return bufs.take(self.E.reshape(-1, 128), self._index(self.ct_pos, self.a)).reshape(self.ng, self.d, 128)


def _plan_for(engine, key_attrs, d, ct_attrs, E, e_prime):
    return (_RowsPlan if _is_rows(ct_attrs) else _Plan)(engine, key_attrs, d, ct_attrs, E, e_prime)


def decrypt_batch(engine, key, d, ct_attrs, E, e_prime):
    """Small universe.  key = (attrs, D): the key's attribute list and its components D_i = g1^(q(i) / t_i), [len(attrs), 64] host
    bytes; ct_attrs: [n][a] attribute values (Python ints); E: [n, a, 128] the components E_i = T_i^s in the order of ct_attrs;
    e_prime: [n, 384].  Returns (messages [n, 384], ok [n]); a ciphertext with fewer than d common attributes has ok = 0 and an
    all-zero row, as the unmarshal entries do, and takes no part in the engine calls (fr_lagrange_basis, g1_scalar_mul,
    multi_pair with one segment of d pairs per ciphertext, gt_div).

    Rows form: ct_attrs a [n, a, 32] uint8 array or CUDA tensor of scalar rows (attribute_rows makes them from integers), of the kind E
    is.  attrs is then [m, 32] rows or a list of integers (converted once), D [m, 64]; or a key per item — attrs [n, m, 32] with
    D [n, m, 64] — for n (key, ciphertext) pairs.  The selection is engine.fr_find_common; messages and ok are those of the integer form."""
    attrs, D = key
    p = _plan_for(engine, attrs, d, ct_attrs, E, e_prime)
    if not p.ng:
        return p.scatter(None)
    P = engine.g1_scalar_mul(bufs.flat(p.key_rows(D, 64)), bufs.flat(p.delta))
    den = engine.multi_pair(bufs.flat(P), bufs.flat(p.ct_rows()), p.seg(d))
    return p.scatter(engine.gt_div(p.rows(p.e_prime), den))


def decrypt_batch_large(engine, key, d, ct_attrs, E, e_pp, e_prime):
    """Large universe.  key = (attrs, d_i [len(attrs), 64], D_i [len(attrs), 128]) with d_i = g1^r_i, D_i = g2^q(i) T_i^r_i; E as in
    decrypt_batch; e_pp: [n, 64] the components E'' = g1^s; e_prime: [n, 384].  One segment of 2 d pairs per ciphertext,
    ([Delta_i] d_i, E_i) ... ([-Delta_i] E'', D_i) ..., with -Delta from engine.fr_neg on the same scalars, then gt_mul.  (The form with
    d + 1 pairs, which sums [Delta_i] D_i in G2 per ciphertext, is not built.)  The rows form is decrypt_batch's, with d_i [m, 64] and
    D_i [m, 128], or [n, m, 64] and [n, m, 128] with a key per item."""
    attrs, di, Di = key
    p = _plan_for(engine, attrs, d, ct_attrs, E, e_prime)
    if bufs.nbytes(e_pp) != p.n * 64 or bufs.is_torch(e_pp) != bufs.is_torch(p.E):
        raise ValueError("e_pp must hold n G1 points of the kind E is")
    if not p.ng:
        return p.scatter(None)
    ng = p.ng
    epp = bufs.expand(p.rows(bufs.view(e_pp, p.n, 64)).reshape(ng, 1, 64), ng, d, 64)
    bases = bufs.cat([p.key_rows(di, 64), epp], 1)                                             # [ng, 2 d, 64]
    delta = p.delta.reshape(ng, d, 32)
    scalars = bufs.cat([delta, engine.fr_neg(bufs.flat(delta)).reshape(ng, d, 32)], 1)
    P = engine.g1_scalar_mul(bufs.flat(bases), bufs.flat(scalars))
    Q = bufs.cat([p.ct_rows(), p.key_rows(Di, 128)], 1)
    return p.scatter(engine.gt_mul(p.rows(p.e_prime), engine.multi_pair(bufs.flat(P), bufs.flat(Q), p.seg(2 * d))))


def compute_t(engine, table, n, xs, nodes=None):
    """T_x = g2^(x^n) * prod_i t_i^Delta(node_i) for every attribute x of xs (computeT, sw05_fibe_large_universe.go:302-325): [k, 128].
    table: a G2 FixedBase over [g2, t_0 ... t_n]; xs: k attribute values (Python ints, scalar rows, or a CUDA tensor of rows).
    A row of scalars is [x^n, Delta_{x,N}(node_0) ... Delta_{x,N}(node_n)] over the ONE set N = {1 ... n+1}: fr_lagrange_basis with a
    shared set, a shared node list and x per row; x^n by square-and-multiply in fr_mul calls; then one table.msm.

    nodes defaults to the reference's own list, 0 ... n — NOT the set: its loop index is used as the node (:315-318), so node 0 lies
    outside N and keeps all n + 1 factors, and the element n + 1 of N is never a node.  Keys and ciphertexts made with the paper's
    nodes 1 ... n+1 do not interoperate with the reference's, which is why the nodes are an argument and not derived from the set."""
    n = int(n)
    if n < 1 or n + 1 > 1024:
        raise ValueError("n must be in 1 .. 1023 (got %d)" % n)
    nodes = list(range(n + 1)) if nodes is None else [int(v) for v in nodes]
    if len(nodes) != n + 1 or table.nbase != n + 2:
        raise ValueError("need n + 1 = %d nodes and a table of n + 2 bases" % (n + 1))
    if not _plan.is_buffer(xs):
        xs = _plan.scalar_rows(xs)
    xs = bufs.view(xs, -1, 32)
    k = xs.shape[0]

    def put(a):
        return bufs.put(a, xs)
    flat = bufs.flat(xs)
    delta = engine.fr_lagrange_basis(put(_plan.scalar_rows(range(1, n + 2))).reshape(-1), n + 1, put(_plan.scalar_rows(nodes)).reshape(-1), n + 1, flat).reshape(k, n + 1, 32)
    acc = engine.fr_mul(flat, put(_plan.scalar_rows([1])).reshape(-1))                         # x, canonical
    base = acc
    for bit in bin(n)[3:]:
        acc = engine.fr_mul(bufs.flat(acc), bufs.flat(acc))
        if bit == "1":
            acc = engine.fr_mul(bufs.flat(acc), bufs.flat(base))
    scalars = bufs.cat([acc.reshape(k, 1, 32), delta], 1)
    return table.msm(bufs.flat(scalars)).reshape(k, 128)


# ------------------------------------------------------------------------------------------------ KeyGenerate
# fibe/sw05_fibe_common.go:205-210 and fibe/sw05_fibe_large_universe.go:153-167: a random polynomial q of degree d - 1 with q(0) = y per user
# (utils.GenerateRandomPolynomial) and utils.ComputePolynomialValue(q, i) per attribute i — engine.fr_poly_eval, k users x m attributes in
# one launch.  The randomness is passed in.  Ragged attribute counts are the caller's to group: rows are rectangular.
def _matrix(x, like, what):
    """(buffer [rows, cols, 32], rows, cols) of a scalar matrix: nested Python ints [rows][cols], or a [rows, cols, 32] uint8 array / tensor"""
    if not _plan.is_buffer(x):
        grid = [list(r) for r in x]
        cols = len(grid[0]) if grid else 0
        if any(len(r) != cols for r in grid):
            raise ValueError("%s: every row needs %d scalars" % (what, cols))
        x = _plan.scalar_rows(grid).reshape(len(grid), cols, 32)
        if like is not None:
            x = bufs.put(x, like)
    if len(x.shape) != 3 or x.shape[2] != 32:
        raise ValueError("%s must be [rows, columns, 32] scalar rows" % what)
    return x, int(x.shape[0]), int(x.shape[1])


def _shares(engine, y, coeffs, attrs):
    """q_j(attrs[j][i]) for the k polynomials y + coeffs[j][0] X + ...: ([k, m, 32], attrs [k, m, 32], k, m)"""
    tensor = next((v for v in (attrs, coeffs) if bufs.is_torch(v)), None)
    attrs, k, m = _matrix(attrs, tensor, "attrs")
    coeffs, kc, dm1 = _matrix(coeffs if coeffs is not None else bufs.empty((k, 0, 32), attrs), attrs, "coeffs")
    if kc != k:
        raise ValueError("coeffs needs one row per user (got %d, k = %d)" % (kc, k))
    bufs.device_of(attrs, coeffs)
    y = bufs.put(_plan.scalar_rows(y) if isinstance(y, int) else np.array(y, dtype=np.uint8, copy=True).reshape(1, 32), attrs)
    rows = bufs.cat([bufs.expand(bufs.view(y, 1, 1, 32), k, 1, 32), coeffs], 1)                     # [k, d, 32]: q_j, constant term first
    q = engine.fr_poly_eval(bufs.flat(rows), bufs.flat(attrs), dm1 + 1, m)
    return bufs.view(q, k, m, 32), attrs, k, m


def keygen_batch(engine, y, coeffs, attrs, t):
    """Small universe, k users of m attributes each.  y: the master secret (an int or 32 bytes); coeffs: [k, d - 1] scalars, the
    coefficients of X^1 .. X^(d-1) of every user's polynomial (d == 1: no columns, or None); attrs: [k, m] attribute values;
    t: [k, m] the master t_i of every attribute.  Scalars are nested Python ints or [k, columns, 32] uint8 arrays / CUDA tensors.
    Returns D [k, m, 64] with D_i = g1^(q(i) / t_i): fr_poly_eval, fr_inverse, fr_mul, generator multiplications."""
    q, attrs, k, m = _shares(engine, y, coeffs, attrs)
    t, kt, mt = _matrix(t, attrs, "t")
    if (kt, mt) != (k, m):
        raise ValueError("t must be [%d, %d] like attrs" % (k, m))
    e = engine.fr_mul(bufs.flat(q), bufs.flat(engine.fr_inverse(bufs.flat(t))))
    return bufs.view(engine.g1_scalar_mul_base(bufs.flat(e)), k, m, 64)


def keygen_batch_large(engine, table, n, y, coeffs, attrs, r):
    """Large universe.  table, n: as for compute_t; y, coeffs, attrs as for keygen_batch; r: [k, m] scalars, the r_i of every attribute.
    Returns (d [k, m, 64], D [k, m, 128]) with d_i = g1^(r_i) and D_i = g2^(q(i)) + [r_i] T_i, T_i = compute_t of the attribute."""
    q, attrs, k, m = _shares(engine, y, coeffs, attrs)
    r, kr, mr = _matrix(r, attrs, "r")
    if (kr, mr) != (k, m):
        raise ValueError("r must be [%d, %d] like attrs" % (k, m))
    T = compute_t(engine, table, n, bufs.view(bufs.flat(attrs), k * m, 32))
    D = engine.g2_add(bufs.flat(engine.g2_scalar_mul_base(bufs.flat(q))), bufs.flat(engine.g2_scalar_mul(bufs.flat(T), bufs.flat(r))))
    return bufs.view(engine.g1_scalar_mul_base(bufs.flat(r)), k, m, 64), bufs.view(D, k, m, 128)


def _seeded_polynomials(attrs, other, d, rng):
    """(attrs [k, m, 32] as a buffer, coeffs [k, d - 1, 32] drawn from rng or None for d == 1, k, m); the buffers are tensors where
    attrs or `other` is one"""
    if not isinstance(d, (int, np.integer)) or isinstance(d, bool) or d < 1:
        raise ValueError("d must be an integer >= 1 (got %s)" % (d,))
    attrs, k, m = _matrix(attrs, next((v for v in (attrs, other) if bufs.is_torch(v)), None), "attrs")
    return attrs, (rng.scalars(attrs, k, int(d) - 1) if d > 1 else None), k, m


def keygen_batch_seeded(engine, y, d, attrs, t, rng):
    """keygen_batch with its randomness drawn on the device: d is the threshold (the polynomials have degree d - 1), rng an
    rng.Randomness over the engine, y, attrs and t as there; returns exactly keygen_batch's D on the coefficients drawn.  The one draw
    (the order is part of the interface): coeffs [k, d - 1], user-major — one stream id, none when d == 1 or k == 0.  The coefficients
    are of the kind of attrs (or of t, where attrs are Python integers).  The seed is key material: whoever holds it can recompute every
    user's polynomial."""
    attrs, coeffs, _, _ = _seeded_polynomials(attrs, t, d, rng)
    return keygen_batch(engine, y, coeffs, attrs, t)


def keygen_batch_large_seeded(engine, table, n, y, d, attrs, rng):
    """keygen_batch_large with its randomness drawn on the device: d, rng as for keygen_batch_seeded, the rest as there; returns exactly
    keygen_batch_large's (d, D) on the scalars drawn.  The draws, in this order (the order is part of the interface): coeffs [k, d - 1],
    then r [k, m] — two stream ids, one when d == 1, none when k == 0.  The seed is key material: whoever holds it can recompute every
    user's polynomial and every r_i."""
    attrs, coeffs, k, m = _seeded_polynomials(attrs, None, d, rng)
    r = rng.scalars(attrs, k, m)
    return keygen_batch_large(engine, table, n, y, coeffs, attrs, r)
