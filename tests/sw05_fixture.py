"""Test helper: Sahai-Waters 2005 fuzzy IBE instances (fibe/sw05_fibe_common.go, fibe/sw05_fibe_large_universe.go) built from known
secrets with any engine that has the bn254 module's function names — SetUp, KeyGenerate and Encrypt restated on exponents: every
group element is ONE multiplication of a generator by the exponent the reference's sequence arrives at (canonical bytes, so the
same element), through engine entries OTHER than the ones under test (pair_batch, gt_exp, g1 / g2 scalar multiplication of a
shared base).  The large-universe T_x shares nothing with sw05.compute_t: t_j = [tau_j] g2 for known tau_j, the exponent
x^n + sum_j tau_j Delta_{x,N}(j) in Python integers (the reference's node list j = 0 .. n over N = 1 .. n+1), one generator
multiplication.

Also here: the reference's FindCommonAttributes and Decrypt loops written out (Python integers, oracle calls).  The stand-in engine
the plan tests run the planner on is tests/standin_engine.py (fr_lagrange_basis from lagrange() below).

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
