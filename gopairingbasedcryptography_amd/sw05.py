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
device, and only ok (n bytes) comes back to the host — the call's one wait.  Both forms give the same bytes.

Below KeyGenerate: the attribute universe of the small construction (Universe: membership and position of every attribute of a batch,
isValidAttributes of fibe/is_valid_attributes.go), SetUp and Encrypt of both universes (sw05_fibe_common.go:147-184, 237-270;
sw05_fibe_large_universe.go:107-135, 199-230), KeyGenerate with the t_i looked up, and the large-universe Decrypt with d + 1 pairs."""
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
    d + 1 pairs, which sums [Delta_i] D_i in G2 per ciphertext, is decrypt_batch_large_msm below: opt-in, the same bytes.)  The rows form
    is decrypt_batch's, with d_i [m, 64] and D_i [m, 128], or [n, m, 64] and [n, m, 128] with a key per item."""
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


# ------------------------------------------------------------------------------------------------ the universe (small construction)
# fibe/sw05_fibe_common.go:81-139: the instance keeps the universe as a map from field element to nothing, and KeyGenerate and Encrypt
# refuse an attribute list with an element outside it (fibe/is_valid_attributes.go).  Here the universe is an ordered list — the order
# its constructor met the values in — and an attribute's position in it is the row of its t_i and T_i.
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
INDEX_NONE = _plan.INDEX_NONE        # Universe.lookup's "not in the universe"


def _canonical(engine, rows):
    """[k, 32] scalar rows of any value below 2^256 reduced modulo r — engine.fr_mul by 1, as compute_t reduces its x"""
    return bufs.view(engine.fr_mul(bufs.flat(rows), bufs.put(_plan.scalar_rows([1]), rows).reshape(-1)), -1, 32)


class Universe:
    """The attribute universe U of a small-universe instance: `size` distinct field elements in a fixed order, `rows` [size, 32] their
    canonical scalar rows (a host array: the universe is public and small).  Made by from_values, from_int64 or range."""

    def __init__(self, values, span=None):
        values = list(values)
        if len(values) >= _plan.INDEX_NONE:
            raise ValueError("a universe holds fewer than 2^32 - 1 attributes")
        self.rows, self.size, self._span = _plan.scalar_rows(values), len(values), span

    @classmethod
    def from_values(cls, values):
        """NewSW05FIBEInstanceByElements: Python ints, or scalar rows [U, 32] (an array or a tensor), reduced modulo r; a value that
        comes again collapses into its first occurrence, as the keys of the reference's map do"""
        if _plan.is_buffer(values) and str(values.dtype) in ("uint8", "torch.uint8"):
            values = [int.from_bytes(v.tobytes(), "little") for v in np.asarray(_plan.host(values), dtype=np.uint8).reshape(-1, 32)]
        return cls(dict.fromkeys(int(v) % R_ORDER for v in values))

    @classmethod
    def from_int64(cls, values):
        """NewSW05FIBEInstanceByInt64Slice: a negative value v stands for r - |v|, as fr.Element.SetInt64 makes it"""
        values = [int(v) for v in values]
        if any(not INT64_MIN <= v <= INT64_MAX for v in values):
            raise ValueError("the values must be 64-bit signed integers")
        return cls(dict.fromkeys(v % R_ORDER for v in values))

    @classmethod
    def range(cls, start, end):
        """NewSW05FIBEInstanceByInt64Pair: the integers start .. end - 1 (none when end <= start), negative ones as from_int64 reads them"""
        start, end = int(start), int(end)
        if not INT64_MIN <= start <= INT64_MAX or not INT64_MIN <= end <= INT64_MAX:
            raise ValueError("start and end must be 64-bit signed integers")
        end = max(start, end)
        return cls((v % R_ORDER for v in range(start, end)), span=(start, end) if start >= 0 else None)

    def lookup(self, engine, attrs):
        """(index [k, a], ok [k] uint8) for k attribute lists of `a` attributes each: attrs is [k, a, 32] scalar rows — an array or a CUDA
        tensor, any value below 2^256, compared modulo r — or nested Python ints [k][a] (host arrays out).  index is the attribute's
        position in `rows`, or INDEX_NONE for one outside the universe, as FixedBase.indexed takes an index table: uint32 on the host,
        the same bits as int32 on the device.  ok = 1 iff every attribute of the list is in the universe (isValidAttributes).

        One engine call, fr_mul by 1 for the canonical rows.  A range universe from a non-negative start is then arithmetic on the low
        8 bytes; any other has its rows and the k * a queries grouped by value together (_buffers.group_rows: numpy.unique /
        torch.unique over the rows) and every group mapped to the universe position it holds, if any.  No loop per attribute and no
        size cap; on a CUDA tensor the grouping waits for the stream once (the count of distinct values)."""
        attrs, k, a = _matrix(attrs, None, "attrs")
        if str(attrs.dtype) not in ("uint8", "torch.uint8"):
            raise ValueError("attrs must be uint8 scalar rows")
        if not k * a:
            return bufs.index_rows_ok(bufs.put(np.zeros(0, dtype=np.int64), attrs), k, a)
        x = _canonical(engine, bufs.view(attrs, k * a, 32))
        if self._span is not None:
            return bufs.index_rows_ok(bufs.range_positions(x, *self._span), k, a)
        distinct, inverse = bufs.group_rows(bufs.cat([bufs.put(self.rows, x), x]))
        first = bufs.put(np.full(int(distinct.shape[0]), -1, dtype=np.int64), x)
        first[inverse[:self.size]] = bufs.put(np.arange(self.size, dtype=np.int64), x)          # the universe's rows are distinct
        return bufs.index_rows_ok(first[inverse[self.size:]], k, a)


# ------------------------------------------------------------------------------------------------ SetUp, KeyGenerate by lookup, Encrypt (small universe)
def _power_of_pairing(engine, y, like, gt_table):
    """e(g1, g2)^y as bsw07.setup makes e_alpha: pair_batch on the generators and gt_exp, or gt_table.indexed with base 0 = e(g1, g2)"""
    if gt_table is not None:
        return bufs.view(gt_table.indexed(_plan.index_rows(np.array([[0]]), like), y, terms=1)[0], 384)
    g1, g2 = engine.generators()
    e = _plan.public(np.asarray(engine.pair_batch(np.asarray(g1, dtype=np.uint8).reshape(-1), np.asarray(g2, dtype=np.uint8).reshape(-1))), 1, 384, like, "e")
    return bufs.view(engine.gt_exp(bufs.flat(e), y), 384)


def setup(engine, universe, y, t, gt_table=None):
    """(pp, msk) of the small universe from its secrets (SetUp, sw05_fibe_common.go:147-184): pp = {"T": [U, 128] with T_i = [t_i] g2,
    "Y": e(g1, g2)^y (384 B)} and msk = {"y": y (32 B), "t": [U, 32]}, row i belonging to universe.rows[i].  y: one scalar, t: U scalars
    (Python ints, 32-byte rows or CUDA tensors; the values are of their kind).  gt_table: an engine.GTFixedBase whose base 0 is
    e(g1, g2), built once by the caller; Y then comes from its indexed products and is the same bytes.  Engine calls:
    g2_scalar_mul_base, pair_batch on the generators and gt_exp (or gt_table.indexed, one term)."""
    like = _plan.like_of(y, t)
    y, t = _plan.scalars(y, like, 1, "y"), _plan.scalars(t, like, universe.size, "t")
    bufs.device_of(y, t)
    T = bufs.view(engine.g2_scalar_mul_base(t), universe.size, 128) if universe.size else bufs.zeros((0, 128), like)
    return {"T": T, "Y": _power_of_pairing(engine, y, like, gt_table)}, {"y": bufs.view(y, 32), "t": bufs.view(t, universe.size, 32)}


def setup_seeded(engine, universe, rng, like=None, gt_table=None):
    """setup with the secrets drawn on the device: rng is an rng.Randomness over the engine.  The draws, in this order (the order is part
    of the interface: it is what makes the keys reproducible from the seed): t [U], then y — the reference's order, two stream ids, one
    for an empty universe.  The reference draws t_i while it ranges over a Go map, in an order that differs from run to run; here
    t_i belongs to universe.rows[i], in the universe's own order.  like: a buffer of the kind the keys are to be (None: host arrays).
    The seed is key material: whoever holds it holds the master secret key."""
    like = np.zeros(0, dtype=np.uint8) if like is None else like
    t = rng.scalars(like, universe.size)
    y = rng.scalars(like, 1)
    return setup(engine, universe, y, t, gt_table=gt_table)


def _scatter(items, rows, *shape):
    """rows of the items with ok = 1 back into n rows of `shape`, the others all zero"""
    width = int(np.prod(shape, dtype=np.int64))
    return bufs.view(items.scatter(rows, width), items.n, *shape)


def keygen_batch_universe(engine, universe, msk, coeffs, attrs):
    """keygen_batch with the t_i looked up: msk is setup's, coeffs [k, d - 1] and attrs [k, m] as keygen_batch takes them.  Returns
    (D [k, m, 64], ok [k]): a user with an attribute outside the universe has ok = 0 and an all-zero row (the reference's "invalid
    user attributes") and takes no part in keygen_batch, which runs on the valid users with msk's t gathered at universe.lookup's
    positions.  ok comes back to the host once — the call's one wait; a y kept on the device comes with it."""
    tensor = next((v for v in (attrs, coeffs) if bufs.is_torch(v)), None)
    attrs, k, m = _matrix(attrs, tensor, "attrs")
    if coeffs is not None:
        coeffs, kc, _ = _matrix(coeffs, attrs, "coeffs")
        if kc != k:
            raise ValueError("coeffs needs one row per user (got %d, k = %d)" % (kc, k))
    bufs.device_of(attrs, coeffs)
    t = _plan.public(msk["t"], universe.size, 32, attrs, "msk t")
    y = np.array(_plan.host(msk["y"]), dtype=np.uint8, copy=True).reshape(32)
    index, ok = universe.lookup(engine, attrs)
    items = _plan.Good(_plan.host(ok).reshape(k), attrs)
    if not items.count or not m:
        return bufs.zeros((k, m, 64), attrs), ok
    mine = bufs.take(t, bufs.flat(items.rows(index))).reshape(items.count, m, 32)
    D = keygen_batch(engine, y, None if coeffs is None else items.rows(coeffs), items.rows(attrs), mine)
    return _scatter(items, D, m, 64), ok


def keygen_batch_universe_seeded(engine, universe, msk, d, attrs, rng):
    """keygen_batch_universe with its randomness drawn on the device: d is the threshold, rng an rng.Randomness over the engine; returns
    exactly keygen_batch_universe's (D, ok) on the coefficients drawn.  The one draw (the order is part of the interface):
    coeffs [k, d - 1], user-major, a row for EVERY user, valid or not, so that a user's polynomial does not depend on the others'
    validity — one stream id, none when d == 1 or k == 0.  The seed is key material."""
    attrs, coeffs, _, _ = _seeded_polynomials(attrs, None, d, rng)
    return keygen_batch_universe(engine, universe, msk, coeffs, attrs)


def encrypt_table(engine, pp):
    """engine.FixedBase over pp["T"], base i = T_i in the universe's order: what encrypt_batch takes as table=.  The window tables cost
    2 MiB of device memory per attribute of the universe; the caller closes the table."""
    return engine.FixedBase(pp["T"], g2=True)


def _blind(engine, Y, s, messages, n, gt_table):
    """Y^s_j M_j: _plan.blind on Y expanded, or the powers from gt_table (a GTFixedBase whose base 0 is Y) and gt_mul"""
    if gt_table is None:
        return _plan.blind(engine, Y, s, messages, n)
    power, _ = gt_table.indexed(_plan.index_rows(np.array([[0]]), messages), bufs.flat(s), terms=1)
    return engine.gt_mul(bufs.flat(power), bufs.flat(messages))


def _encrypt_args(attrs, messages, s):
    """(attrs [n, a, 32], messages [n, 384], s flat, n, a) of an Encrypt, checked: one kind, one device, a list and a scalar per message"""
    if not _plan.is_buffer(messages):
        raise ValueError("messages must be a uint8 array or a CUDA tensor")
    n = bufs.nbytes(messages) // 384
    if bufs.nbytes(messages) != n * 384:
        raise ValueError("messages must hold whole GT elements")
    attrs, k, a = _matrix(attrs, messages, "attrs")
    bufs.device_of(messages, attrs)
    if k != n:
        raise ValueError("attrs needs one row per message (got %d, n = %d)" % (k, n))
    return attrs, bufs.view(messages, n, 384), _plan.scalars(s, messages, n, "s"), n, a


def encrypt_batch(engine, universe, pp, attrs, messages, s, table=None, gt_table=None):
    """Small universe, n ciphertexts of `a` attributes each (Encrypt, sw05_fibe_common.go:237-270).  pp: setup's; attrs: [n][a] Python
    ints or [n, a, 32] scalar rows; messages [n, 384]; s: n scalars.  Returns (E [n, a, 128], e_prime [n, 384], ok [n]) with
    E[c, i] = [s_c] T_attr(c, i) in the order of attrs and e_prime = M Y^s — the operands of decrypt_batch.  numpy in gives numpy out, CUDA
    tensors give tensors.  A ciphertext with an attribute outside the universe has ok = 0 (the reference's "invalid message
    attributes") and all-zero rows and takes no part in the group operations; ok comes back to the host once, the call's one wait.
    An attribute that comes twice in one list is legal and gives the same point at both positions: the reference's map keeps one of
    them, and FindCommonAttributes uses the first.

    Engine calls: universe.lookup; gt_exp on Y expanded and gt_mul, or with gt_table (an engine.GTFixedBase whose base 0 is Y)
    gt_table.indexed and gt_mul; for E a gather of pp["T"] and g2_scalar_mul with a base per scalar, or with table (encrypt_table(pp),
    opt-in; the same bytes) table.indexed with terms = 1, the index rows being lookup's positions: 32 mixed additions per attribute and
    no doublings."""
    attrs, messages, s, n, a = _encrypt_args(attrs, messages, s)
    U = universe.size
    Y = _plan.public(pp["Y"], 1, 384, messages, "pp Y")
    if table is None:
        T = _plan.public(pp["T"], U, 128, messages, "pp T")
    elif table.nbase != U or not table.g2:
        raise ValueError("the table must be a G2 table over the universe's %d attributes" % U)
    index, ok = universe.lookup(engine, attrs)
    items = _plan.Good(_plan.host(ok).reshape(n), messages)
    ng = items.count
    if not ng:
        return bufs.zeros((n, a, 128), messages), bufs.zeros((n, 384), messages), ok
    sg = items.rows(bufs.view(s, n, 32))
    e_prime = _blind(engine, Y, sg, items.rows(messages), ng, gt_table)
    if not a:
        return bufs.zeros((n, 0, 128), messages), _scatter(items, e_prime, 384), ok
    index, sa = items.rows(index), bufs.flat(bufs.expand(bufs.view(sg, ng, 1, 32), ng, a, 32))
    if table is None:
        E = engine.g2_scalar_mul(bufs.flat(bufs.take(T, bufs.flat(index))), sa)
    else:
        E, _ = table.indexed(bufs.flat(index).reshape(ng * a, 1), sa, terms=1)
    return _scatter(items, E, a, 128), _scatter(items, e_prime, 384), ok


def encrypt_batch_seeded(engine, universe, pp, attrs, messages, rng, table=None, gt_table=None):
    """encrypt_batch with its randomness drawn on the device: rng is an rng.Randomness over the engine, everything else as there, and the
    return value is exactly encrypt_batch's on the scalars drawn.  The one draw: s [n], a scalar for EVERY ciphertext, valid or not —
    one stream id, none when n == 0.  The seed is key material: whoever holds it can recompute s and with it every message."""
    s = rng.scalars(messages, bufs.nbytes(messages) // 384)
    return encrypt_batch(engine, universe, pp, attrs, messages, s, table=table, gt_table=gt_table)


# ------------------------------------------------------------------------------------------------ SetUp, the table, Encrypt (large universe)
def setup_large(engine, n, y, tau, gt_table=None):
    """(pp, msk) of the large universe (NewSW05FIBELargeUniverseInstance and SetUp, sw05_fibe_large_universe.go:87-135):
    pp = {"n": n, "t": [n + 1, 128] with t[j] = [tau_j] g2 — the reference's ti[1 .. n+1], ti[j + 1] in row j — and "Y": e(g1, g2)^y},
    msk = {"y": y (32 B)}.  y: one scalar, tau: n + 1 scalars (Python ints, rows or CUDA tensors); gt_table as for setup."""
    n = int(n)
    if n < 1 or n + 1 > 1024:
        raise ValueError("n must be in 1 .. 1023 (got %d)" % n)
    like = _plan.like_of(y, tau)
    y, tau = _plan.scalars(y, like, 1, "y"), _plan.scalars(tau, like, n + 1, "tau")
    bufs.device_of(y, tau)
    pp = {"n": n, "t": bufs.view(engine.g2_scalar_mul_base(tau), n + 1, 128), "Y": _power_of_pairing(engine, y, like, gt_table)}
    return pp, {"y": bufs.view(y, 32)}


def setup_large_seeded(engine, n, rng, like=None, gt_table=None):
    """setup_large with the secrets drawn on the device.  The draws, in this order (the order is part of the interface): y, then
    tau [n + 1] — the reference's order, whose instance draws y when it is made, before SetUp runs.  Two stream ids.  like: a buffer
    of the kind the keys are to be (None: host arrays).  The seed is key material: whoever holds it holds the master secret key."""
    like = np.zeros(0, dtype=np.uint8) if like is None else like
    y = rng.scalars(like, 1)
    tau = rng.scalars(like, int(n) + 1)
    return setup_large(engine, n, y, tau, gt_table=gt_table)


def large_table(engine, pp, nodes=None):
    """(table, nodes): the G2 FixedBase and the node list that compute_t, keygen_batch_large and encrypt_batch_large take, from
    setup_large's pp.  The caller closes the table (2 MiB of device memory per base, n + 2 bases).

    nodes=None reproduces the reference literally (computeT, sw05_fibe_large_universe.go:315-321): its loop index 0 .. n is the node
    AND the key into the map ti, whose keys are 1 .. n+1 — key 0 is absent and reads as the zero value, the point at infinity, and
    ti[n+1] is never read.  The bases are [g2, infinity, ti[1] .. ti[n]] with the nodes 0 .. n.  nodes="paper" is the construction as
    published: the bases [g2, ti[1] .. ti[n+1]] with the nodes 1 .. n+1.  Keys and ciphertexts of the two do not interoperate."""
    n, t = int(pp["n"]), bufs.view(pp["t"], -1, 128)
    if t.shape[0] != n + 1:
        raise ValueError("pp t must hold n + 1 = %d G2 points" % (n + 1))
    g2 = bufs.put(np.array(engine.generators()[1], dtype=np.uint8, copy=True).reshape(1, 128), t)
    if nodes is None:
        bases, nodes = bufs.cat([g2, bufs.zeros((1, 128), t), t[:n]]), list(range(n + 1))
    elif isinstance(nodes, str) and nodes == "paper":
        bases, nodes = bufs.cat([g2, t]), list(range(1, n + 2))
    else:
        raise ValueError('nodes is None (the reference\'s indexing) or "paper"')
    return engine.FixedBase(bufs.flat(bases).reshape(n + 2, 128), g2=True), nodes


FOLD_SCALAR_BYTES = 1 << 28          # the fold route's scalar rows per chunk: 256 MiB, 2^18 outputs at n = 30
# The share of distinct attribute values, distinct / total, below which route="auto" takes the dedupe route.  Measured crossover 0.90 at
# 2^16 ciphertexts x 24 attributes, n = 32 (profiles/sw05_encrypt.json: dedupe 57 ms + 351 ms x share on a straight line through shares
# 0, 0.003, 0.5 and 1, fold 373 ms whatever the share; the estimate from compute_t at 0.24 us per attribute and 29 ns per G2
# multiplication was 0.88).  Both routes give the same bytes, so the constant carries no safety margin.
AUTO_DEDUPE_BELOW = 0.90


def _t_scalars(engine, n, nodes, xs):
    """the scalar rows of computeT for k attribute rows xs [k, 32]: [k, n + 2, 32] = [x^n, Delta_{x,N}(node_0) .. Delta_{x,N}(node_n)]
    over N = {1 .. n+1} — compute_t's own lines restated for the fold route, which multiplies the rows through before the sum"""
    k, flat = xs.shape[0], bufs.flat(xs)
    put = lambda a: bufs.put(a, xs).reshape(-1)
    delta = engine.fr_lagrange_basis(put(_plan.scalar_rows(range(1, n + 2))), n + 1, put(_plan.scalar_rows(nodes)), n + 1, flat).reshape(k, n + 1, 32)
    acc = base = engine.fr_mul(flat, put(_plan.scalar_rows([1])))
    for bit in bin(n)[3:]:
        acc = engine.fr_mul(bufs.flat(acc), bufs.flat(acc))
        if bit == "1":
            acc = engine.fr_mul(bufs.flat(acc), bufs.flat(base))
    return bufs.cat([acc.reshape(k, 1, 32), delta], 1)


def encrypt_batch_large(engine, table, n, pp, attrs, messages, s, nodes=None, route="auto", gt_table=None):
    """Large universe, k ciphertexts of `a` attributes each (Encrypt, sw05_fibe_large_universe.go:199-230).  table, n, nodes: as for
    compute_t (large_table(pp) makes them); pp: setup_large's (its Y is used); attrs: [k][a] Python ints or [k, a, 32] scalar rows;
    messages [k, 384]; s: k scalars.  Returns (E [k, a, 128], e_pp [k, 64], e_prime [k, 384]) with E[c, i] = [s_c] T_x for
    x = attrs[c][i], e_pp = [s] g1 and e_prime = M Y^s — the operands of decrypt_batch_large.  Any field element is an attribute: there
    is no universe to check, as in the reference.  gt_table: an engine.GTFixedBase whose base 0 is Y.

    E by two routes that give the same bytes:
      "dedupe"  the k * a values reduced (fr_mul by 1) and grouped by value (_buffers.group_rows: one wait for the stream), compute_t once
                per DISTINCT value, a gather, and g2_scalar_mul with a base per scalar;
      "fold"    the scalar row of compute_t multiplied through by s_c (fr_mul on s expanded) and one table.msm per output:
                [s] T_x = [s x^n] g2 + sum_j [s Delta_j] t_j, no intermediate T_x and no variable-base multiplication.  The outputs go
                through in chunks whose scalar rows, (n + 2) * 32 bytes per output, stay within FOLD_SCALAR_BYTES = 256 MiB (the
                multiplied-through copy and the expanded s are as large again);
      "auto"    groups as dedupe does and takes dedupe when distinct / total < AUTO_DEDUPE_BELOW, else fold."""
    n = int(n)
    if route not in ("auto", "dedupe", "fold"):
        raise ValueError('route is "auto", "dedupe" or "fold" (got %r)' % (route,))
    if n < 1 or n + 1 > 1024:
        raise ValueError("n must be in 1 .. 1023 (got %d)" % n)
    nodes = list(range(n + 1)) if nodes is None else [int(v) for v in nodes]
    if len(nodes) != n + 1 or table.nbase != n + 2 or int(pp["n"]) != n:
        raise ValueError("need n + 1 = %d nodes, a table of n + 2 bases and the pp of this n" % (n + 1))
    attrs, messages, s, k, a = _encrypt_args(attrs, messages, s)
    Y = _plan.public(pp["Y"], 1, 384, messages, "pp Y")
    if not k:
        return bufs.zeros((0, a, 128), messages), bufs.zeros((0, 64), messages), bufs.zeros((0, 384), messages)
    e_pp = bufs.view(engine.g1_scalar_mul_base(s), k, 64)
    e_prime = bufs.view(_blind(engine, Y, s, messages, k, gt_table), k, 384)
    rows = k * a
    if not rows:
        return bufs.zeros((k, 0, 128), messages), e_pp, e_prime
    xs, sa = bufs.view(attrs, rows, 32), bufs.expand(bufs.view(s, k, 1, 32), k, a, 32).reshape(rows, 32)
    if route != "fold":
        distinct, inverse = bufs.group_rows(_canonical(engine, xs))
        if route == "auto":
            route = "dedupe" if distinct.shape[0] < AUTO_DEDUPE_BELOW * rows else "fold"
    if route == "dedupe":
        T = compute_t(engine, table, n, distinct, nodes)
        E = engine.g2_scalar_mul(bufs.flat(bufs.take(T, inverse)), bufs.flat(sa))
    else:
        chunk = max(1, FOLD_SCALAR_BYTES // ((n + 2) * 32))
        parts = []
        for lo in range(0, rows, chunk):
            hi = min(rows, lo + chunk)
            sx = bufs.expand(sa[lo:hi].reshape(hi - lo, 1, 32), hi - lo, n + 2, 32)
            folded = engine.fr_mul(bufs.flat(_t_scalars(engine, n, nodes, xs[lo:hi])), bufs.flat(sx))
            parts.append(bufs.view(table.msm(bufs.flat(folded)), hi - lo, 128))
        E = parts[0] if len(parts) == 1 else bufs.cat(parts)
    return bufs.view(E, k, a, 128), e_pp, e_prime


def encrypt_batch_large_seeded(engine, table, n, pp, attrs, messages, rng, nodes=None, route="auto", gt_table=None):
    """encrypt_batch_large with its randomness drawn on the device: exactly its return value on the scalars drawn.  The one draw: s [k] —
    one stream id, none when k == 0.  The seed is key material: whoever holds it can recompute s and with it every message."""
    s = rng.scalars(messages, bufs.nbytes(messages) // 384)
    return encrypt_batch_large(engine, table, n, pp, attrs, messages, s, nodes=nodes, route=route, gt_table=gt_table)


def decrypt_batch_large_msm(engine, key, d, ct_attrs, E, e_pp, e_prime):
    """decrypt_batch_large with the d pairings against E'' folded into one: per ciphertext S = -sum_i [Delta_i] D_i from
    engine.g2_multi_scalar_mul over segments of d (the scalars engine.fr_neg of the Delta) and ONE segment of d + 1 pairs,
    ([Delta_i] d_i, E_i) ..., (E'', S) — d multiplications in G1 where decrypt_batch_large does 2 d, as lw11.decrypt_batch_msm folds its
    pairings against H(GID).  The arguments, the messages and ok are decrypt_batch_large's, byte for byte (bilinearity, canonical GT
    output), in both input forms.  Opt-in: decrypt_batch_large stays the default."""
    attrs, di, Di = key
    p = _plan_for(engine, attrs, d, ct_attrs, E, e_prime)
    if bufs.nbytes(e_pp) != p.n * 64 or bufs.is_torch(e_pp) != bufs.is_torch(p.E):
        raise ValueError("e_pp must hold n G1 points of the kind E is")
    if not p.ng:
        return p.scatter(None)
    ng = p.ng
    S = engine.g2_multi_scalar_mul(bufs.flat(p.key_rows(Di, 128)), engine.fr_neg(bufs.flat(p.delta)), p.seg(d))
    folded = engine.g1_scalar_mul(bufs.flat(p.key_rows(di, 64)), bufs.flat(p.delta))
    P = bufs.cat([bufs.view(folded, ng, d, 64), p.rows(bufs.view(e_pp, p.n, 64)).reshape(ng, 1, 64)], 1)
    Q = bufs.cat([p.ct_rows(), bufs.view(S, ng, 1, 128)], 1)
    return p.scatter(engine.gt_mul(p.rows(p.e_prime), engine.multi_pair(bufs.flat(P), bufs.flat(Q), p.seg(d + 1))))
