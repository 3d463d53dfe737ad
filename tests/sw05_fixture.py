"""Test helper: Sahai-Waters 2005 fuzzy IBE instances (fibe/sw05_fibe_common.go, fibe/sw05_fibe_large_universe.go) built from known
secrets with any engine that has the bn254 module's function names — SetUp, KeyGenerate and Encrypt restated on exponents: every
group element is ONE multiplication of a generator by the exponent the reference's sequence arrives at (canonical bytes, so the
same element), through engine entries OTHER than the ones under test (pair_batch, gt_exp, g1 / g2 scalar multiplication of a
shared base).  The large-universe T_x shares nothing with sw05.compute_t: t_j = [tau_j] g2 for known tau_j, the exponent
x^n + sum_j tau_j Delta_{x,N}(j) in Python integers (the reference's node list j = 0 .. n over N = 1 .. n+1), one generator
multiplication.

Also here: the reference's FindCommonAttributes and Decrypt loops written out (Python integers, oracle calls), and the stand-ins the
plan tests run the planner on (OracleEngine with fr_lagrange_basis in Python integers, OracleTable for FixedBase, and TensorEngine,
which lets any of the plan tests' stand-ins take CPU tensors so that a planner's tensor path runs without a GPU).

numpy arrays by default; with `dev` a torch device everything per ciphertext is made and kept in HBM (the instances at size)."""
import numpy as np

import bn254_py as o

R = o.R


def sc(tag, i=0):
    return o.bench_scalar("sw05-" + tag, i)


def kbytes(vals):
    return np.frombuffer(b"".join((int(v) % R).to_bytes(32, "little") for v in vals), dtype=np.uint8)


def kints(buf):
    return [int.from_bytes(r.tobytes(), "little") for r in np.asarray(buf, dtype=np.uint8).reshape(-1, 32)]


def lagrange(i, S, x):
    """utils.ComputeLagrangeBasis(i, S, x): the loop of the reference, one inversion per factor"""
    res = 1
    for j in S:
        if j % R != i % R:
            res = res * ((x - j) % R) * pow((i - j) % R, -1, R) % R
    return res


def lagrange_one_inversion(i, S, x):
    """the same value with numerator and denominator multiplied out first (the fixture's T_x at size: one inversion per coefficient)"""
    num = den = 1
    for j in S:
        if j % R != i % R:
            num, den = num * (x - j) % R, den * (i - j) % R
    return num * pow(den, -1, R) % R


def find_common(attrs1, attrs2, required):
    """utils/find_common_attributes.go restated: a map of attrs1, a walk over attrs2 with a set against repeats, the first
    `required` of what was found or None"""
    have = {a % R: True for a in attrs1}
    common, seen = [], {}
    for a in attrs2:
        if have.get(a % R) and not seen.get(a % R):
            common.append(a % R)
            seen[a % R] = True
    return common[:required] if len(common) >= required else None


def t_exponent(taus, n, x, nodes=None):
    """log_g2 of computeT(x): x^n + sum_j tau_j Delta_{x,N}(node_j), N = {1 .. n+1}, nodes 0 .. n unless given"""
    N = list(range(1, n + 2))
    nodes = list(range(n + 1)) if nodes is None else nodes
    return (pow(x, n, R) + sum(t * lagrange_one_inversion(j, N, x) for t, j in zip(taus, nodes))) % R


class Instance:
    """one key (key_attrs) and len(ct_attrs) ciphertexts.  Small universe: key = (attrs, D).  Large (n_univ = n): key = (attrs, d, D),
    plus e_pp and the bases [g2, t_0 .. t_n] of the table.  E: [n_ct, a, 128], e_prime: [n_ct, 384], msgs: [n_ct, 384]."""

    def __init__(self, eng, d, key_attrs, ct_attrs, n_univ=None, dev=None, tag=""):
        self.eng, self.d, self.key_attrs, self.ct_attrs, self.n_univ, self.dev = eng, d, list(key_attrs), [list(c) for c in ct_attrs], n_univ, dev
        if dev is not None:
            import torch
            put = lambda a: torch.from_numpy(np.array(a, dtype=np.uint8, copy=True)).to(dev)
        else:
            put = lambda a: np.array(a, dtype=np.uint8, copy=True)
        host = lambda a: np.asarray(a.cpu().numpy() if dev is not None else a)
        g1, g2 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8), np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
        self.g2 = g2
        e = np.asarray(eng.pair_batch(g1, g2)).reshape(1, 384)
        y = sc(tag + "y")
        poly = [y] + [sc(tag + "q", j) for j in range(1, d)]                                  # q of degree d - 1, q(0) = y
        q = lambda i: sum(c * pow(i, j, R) for j, c in enumerate(poly)) % R
        n_ct = len(ct_attrs)
        s = [sc(tag + "s", t) for t in range(n_ct)]
        msg = [sc(tag + "msg", t) for t in range(n_ct)]
        gexp = lambda ks: eng.gt_exp(put(np.tile(e, (len(ks), 1))), put(kbytes(ks)))
        g1mul = lambda ks: eng.g1_scalar_mul(put(g1), put(kbytes(ks)))
        g2mul = lambda ks: eng.g2_scalar_mul(put(g2), put(kbytes(ks)))
        self.msgs = gexp(msg)                                                                 # M_t = e(g1, g2)^msg_t
        self.e_prime = gexp([(m + y * st) % R for m, st in zip(msg, s)])                      # M Y^s
        universe = sorted({a % R for a in self.key_attrs} | {a % R for c in self.ct_attrs for a in c})
        if n_univ is None:
            t = {a: sc(tag + "t", k) for k, a in enumerate(universe)}                         # T_i = g2^t_i
            self.key = (self.key_attrs, host(g1mul([q(i) * pow(t[i % R], -1, R) for i in self.key_attrs])).reshape(-1, 64))      # D_i = g1^(q(i) / t_i)
        else:
            self.taus = [sc(tag + "tau", j) for j in range(n_univ + 1)]
            self.table_bases = np.concatenate([g2.reshape(1, 128), host(g2mul(self.taus)).reshape(-1, 128)])
            t = {a: t_exponent(self.taus, n_univ, a) for a in universe}                       # T_i = g2^t(i)
            r = [sc(tag + "r", k) for k in range(len(self.key_attrs))]
            self.key = (self.key_attrs, host(g1mul(r)).reshape(-1, 64),                       # d_i = g1^r_i, D_i = g2^q(i) T_i^r_i
                        host(g2mul([(q(i) + t[i % R] * ri) % R for i, ri in zip(self.key_attrs, r)])).reshape(-1, 128))
            self.e_pp = g1mul(s)                                                              # E'' = g1^s
        self.t = t
        self.E = g2mul([t[a % R] * st % R for c, st in zip(self.ct_attrs, s) for a in c]).reshape(n_ct, -1, 128)      # E_i = T_i^s

    def decryptable(self):
        return [find_common(self.key_attrs, c, self.d) is not None for c in self.ct_attrs]

    def reference_shaped_decrypt(self, oracle, t):
        """Decrypt of the reference with oracle calls: one Pair (two in the large universe, and a Div) per common attribute, GT.Exp by
        ComputeLagrangeBasis(i, S, 0), the running product, then Div (small) or Mul (large).  None where the reference fails."""
        host = lambda a: np.asarray(a.cpu().numpy() if self.dev is not None else a)
        S = find_common(self.key_attrs, self.ct_attrs[t], self.d)
        if S is None:
            return None
        kpos = {a % R: p for p, a in reversed(list(enumerate(self.key_attrs)))}
        cpos = {a % R: p for p, a in reversed(list(enumerate(self.ct_attrs[t])))}
        E, e_prime = host(self.E[t]), host(self.e_prime.reshape(-1, 384)[t])
        den = np.frombuffer(o.gt_to_bytes(o.F12_ONE), dtype=np.uint8)
        for i in S:
            if self.n_univ is None:
                term = oracle.pair_batch(self.key[1][kpos[i]], E[cpos[i]])[0]
            else:
                term = oracle.gt_div(oracle.pair_batch(self.key[1][kpos[i]], E[cpos[i]])[0],
                                     oracle.pair_batch(host(self.e_pp.reshape(-1, 64)[t]), self.key[2][kpos[i]])[0])[0]
            den = oracle.gt_mul(den, oracle.gt_exp(term, kbytes([lagrange(i, S, 0)]))[0])[0]
        return (oracle.gt_div if self.n_univ is None else oracle.gt_mul)(e_prime, den)[0]


def at_size_attributes(n_ct, a, n_key, d, every, seed=2005):
    """(key_attrs, ct_attrs): a key of n_key attributes and n_ct ciphertexts of `a` attributes each, in shuffled order, with d .. a
    attributes in common — except every `every`-th ciphertext (t % every == every - 1), which shares exactly d - 1.  The attribute
    values mix small integers and full-size field elements."""
    rng = np.random.default_rng(seed)
    value = lambda u: u + 1 if u % 3 else sc("attr", u)
    key = [value(u) for u in range(n_key)]
    other = [value(u) for u in range(n_key, n_key + a)]
    cts = []
    for t in range(n_ct):
        c = d - 1 if t % every == every - 1 else int(rng.integers(d, min(a, n_key) + 1))
        attrs = [key[i] for i in rng.permutation(n_key)[:c]] + [other[i] for i in rng.permutation(a)[:a - c]]
        cts.append([attrs[i] for i in rng.permutation(a)])
    return key, cts


# ------------------------------------------------------------------------------------------------ stand-ins for the plan tests
class OracleEngine:
    """the engine's function names on the oracle (host arrays only); fr_* in Python integers"""

    def __init__(self, oracle):
        self.o = oracle

    def _k(self, ks):
        return kbytes(ks) if isinstance(ks, (list, tuple)) else ks

    def pair_batch(self, P, Q): return self.o.pair_batch(P, Q)
    def multi_pair(self, P, Q, off): return self.o.multi_pair(P, Q, off, threads=4)
    def g1_scalar_mul(self, b, k): return self.o.g1_scalar_mul(b, self._k(k), threads=4)
    def g2_scalar_mul(self, b, k): return self.o.g2_scalar_mul(b, self._k(k), threads=4)
    def gt_mul(self, a, b): return self.o.gt_mul(a, b)
    def gt_div(self, a, b): return self.o.gt_div(a, b)
    def gt_exp(self, x, k): return self.o.gt_exp(x, self._k(k))
    def fr_neg(self, a): return kbytes([-v for v in kints(a)]).reshape(-1, 32)
    def fr_mul(self, a, b):
        a, b = kints(a), kints(b)
        return kbytes([x * b[i if len(b) > 1 else 0] for i, x in enumerate(a)]).reshape(-1, 32)

    def fr_lagrange_basis(self, set, B, nodes=None, m=None, x=None):
        S = np.asarray(kints(set), dtype=object).reshape(-1, B)
        N = S if nodes is None else np.asarray(kints(nodes), dtype=object).reshape(-1, m)
        X = [0] if x is None else kints(x)
        k = max(len(S), len(N), len(X))
        pick = lambda a, j: a[j if len(a) > 1 else 0]
        return kbytes([lagrange(t, list(pick(S, j)), pick(X, j)) for j in range(k) for t in pick(N, j)]).reshape(k, -1, 32)


class OracleTable:
    """FixedBase(bases, g2=True).msm on the oracle: one scalar multiplication per base and a sum per row"""

    def __init__(self, oracle, bases):
        self.o, self.bases = oracle, np.asarray(bases, dtype=np.uint8).reshape(-1, 128)
        self.nbase = self.bases.shape[0]

    def msm(self, scalars):
        k = np.asarray(scalars, dtype=np.uint8).reshape(-1, self.nbase, 32)
        return np.stack([np.asarray(self.o.g2_sum(self.o.g2_scalar_mul(self.bases, row.reshape(-1), threads=4))).reshape(128) for row in k])


class TensorEngine:
    """Any stand-in engine (numpy only) behind the engine's tensor behaviour: tensors among the arguments go in as numpy arrays, and
    a call that was given a tensor hands its array results back as CPU tensors.  A call on host data alone passes through."""

    def __init__(self, engine):
        self._engine = engine

    def __getattr__(self, name):
        fn = getattr(self._engine, name)
        if not callable(fn):
            return fn
        import torch

        def call(*args, **kw):
            tensors = [a for a in list(args) + list(kw.values()) if isinstance(a, torch.Tensor)]
            host = lambda a: a.numpy() if isinstance(a, torch.Tensor) else a
            res = fn(*[host(a) for a in args], **{k: host(v) for k, v in kw.items()})
            if not tensors:
                return res
            back = lambda r: torch.from_numpy(np.array(r, dtype=np.uint8, copy=True)) if isinstance(r, np.ndarray) else r
            return tuple(back(r) for r in res) if isinstance(res, tuple) else back(res)
        return call


def tensors(*arrays):
    """copies of host arrays as CPU uint8 tensors"""
    import torch
    return [torch.from_numpy(np.array(a.cpu() if isinstance(a, torch.Tensor) else a, dtype=np.uint8, copy=True)) for a in arrays]


def same_on_tensors(got, want):
    """the tensor run of a planner returned tensors, of the numpy run's shape, holding the numpy run's bytes"""
    import torch
    assert isinstance(got, torch.Tensor) and isinstance(want, np.ndarray)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    return got.numpy().tobytes() == want.tobytes()
