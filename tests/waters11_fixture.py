"""Test helper: Waters 2011 CP-ABE instances (cpabe/waters11/waters11_cpabe.go:82-237) built from known secrets with any engine that has
the bn254 module's function names — SetUp, KeyGenerate and Encrypt restated on exponents: every group element is ONE multiplication
of a generator by the exponent the reference's ScalarMultiplication / Add sequence arrives at (canonical bytes, so the same
element), through engine entries OTHER than the ones under test (pair_batch, gt_exp, g1 / g2 scalar multiplication of a shared
base).  One key against n ciphertexts, each under a policy of its own, all padded to R rows: a padding row carries a random point
(its weight is 0, so it must not matter).  Encrypt shares over every ROW of the matrix, as the scheme does (the reference's loop runs
to the column count, waters11_cpabe.go:182,211: the same thing for its square test matrices).

Also here: the scheme's Decrypt row by row with oracle calls (each row's own term raised to its own weight), the policies of the
tests.  The stand-in engine the plan tests run the planner on is tests/standin_engine.py.

numpy arrays by default; with `dev` a torch device everything per ciphertext is made and kept in HBM (the instances at size)."""
import numpy as np

import bn254_py as o
import lw11_fixture as lf
from sw05_fixture import kbytes
from gopairingbasedcryptography_amd import lw11

R = o.R


def sc(tag, i=0):
    return o.bench_scalar("w11-" + tag, i)


def and_or_16():
    """(A1 and ... and A8) or (B1 and ... and B8): two AND chains of 8 rows sharing column 0, 16 rows x 15 columns"""
    m = [[0] * 15 for _ in range(16)]
    for half in range(2):
        base = 1 + 7 * half                                  # the chain's own columns base .. base + 6
        for i in range(8):
            x = 8 * half + i
            if i == 0:
                m[x][0] = 1
                m[x][base] = 1
            else:
                m[x][base + i - 1] = -1
                if i < 7:
                    m[x][base + i] = 1
    return m, [300 + x for x in range(16)]


class Instance:
    def __init__(self, eng, key_attrs, policies, rows=None, dev=None, tag=""):
        self.eng, self.key_attrs, self.policies, self.dev = eng, sorted(set(key_attrs)), policies, dev
        n = self.n = len(policies)
        Rr = self.R = max(len(m) for m, _ in policies) if rows is None else rows
        if dev is not None:
            import torch
            put = lambda a: torch.from_numpy(np.array(a, dtype=np.uint8, copy=True)).to(dev)
        else:
            put = lambda a: np.array(a, dtype=np.uint8, copy=True)
        host = lambda a: np.asarray(a.cpu().numpy() if dev is not None else a)
        g1, g2 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8), np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
        e = np.asarray(eng.pair_batch(g1, g2)).reshape(1, 384)
        alpha, a, t = sc(tag + "alpha"), sc(tag + "a"), sc(tag + "t")                      # SetUp, KeyGenerate
        universe = sorted(set(self.key_attrs) | {u for _, rho in policies for u in rho})
        tau = {u: sc(tag + "tau", u) for u in universe}                                    # h_u = g1^tau_u
        gexp = lambda ks: eng.gt_exp(put(np.tile(e, (len(ks), 1))), put(kbytes(ks)))
        g1mul = lambda ks: eng.g1_scalar_mul(put(g1), put(kbytes(ks)))
        g2mul = lambda ks: eng.g2_scalar_mul(put(g2), put(kbytes(ks)))
        kl = host(g1mul([(alpha + a * t) % R] + [tau[u] * t % R for u in self.key_attrs])).reshape(-1, 64)
        self.key = (kl[0].copy(), host(g2mul([t])).reshape(128), {u: kl[1 + i].copy() for i, u in enumerate(self.key_attrs)})
        # Encrypt, per ciphertext: v = (s, v_2, ...), lambda_x = M_x . v, C_x = g1^(a lambda_x) h_rho(x)^(-r_x), D_x = g2^r_x
        s = [sc(tag + "s", j) for j in range(n)]
        msg = [sc(tag + "msg", j) for j in range(n)]
        cexp, rexp = [], []
        for j, (m, rho) in enumerate(policies):
            cols = len(m[0])
            v = [s[j]] + [sc(tag + "v%d" % c, j) for c in range(1, cols)]
            for x in range(Rr):
                rx = sc(tag + "r%d" % x, j)
                rexp.append(rx)
                if x < len(m):
                    lam = sum(int(mv) * vv for mv, vv in zip(m[x], v)) % R
                    cexp.append((a * lam - tau[rho[x]] * rx) % R)
                else:
                    cexp.append(sc(tag + "pad%d" % x, j))                                  # a padding row: anything
        self.msgs = gexp(msg)                                                              # M_j = e(g1, g2)^msg_j
        self.c = gexp([(mj + alpha * sj) % R for mj, sj in zip(msg, s)])                   # M e(g1, g2)^(alpha s)
        self.c_prime = g2mul(s)                                                            # g2^s
        self.cx = g1mul(cexp)
        self.dx = g2mul(rexp)

    def host(self, a):
        return np.asarray(a.cpu().numpy() if self.dev is not None else a)

    def satisfied(self):
        return [lw11.reconstruction_weights(m, rho, self.key_attrs) is not None for m, rho in self.policies]

    def row_by_row_decrypt(self, oracle, j):
        """Decrypt of waters11_cpabe.go:248-290 with oracle calls, one pairing at a time, Mul / Exp / Mul per used row, Div / Div — with
        each row's own weight (the scheme; the reference takes wSlice[i] from the compacted slice).  None where it fails."""
        m, rho = self.policies[j]
        got = lw11.reconstruction_weights(m, rho, self.key_attrs)
        if got is None:
            return None
        K, L, kx = self.key
        cx, dx = self.host(self.cx).reshape(-1, 64)[j * self.R:(j + 1) * self.R], self.host(self.dx).reshape(-1, 128)[j * self.R:(j + 1) * self.R]
        num = oracle.pair_batch(K, self.host(self.c_prime).reshape(-1, 128)[j])[0]
        den = np.frombuffer(o.gt_to_bytes(o.F12_ONE), dtype=np.uint8)
        for x, w in zip(*got):
            term = oracle.gt_mul(oracle.pair_batch(cx[x], L)[0], oracle.pair_batch(kx[rho[x]], dx[x])[0])[0]
            den = oracle.gt_mul(den, oracle.gt_exp(term, kbytes([w]))[0])[0]
        return oracle.gt_div(self.host(self.c).reshape(-1, 384)[j], oracle.gt_div(num, den)[0])[0]


def small_policies():
    """four policies of different shapes and the key that satisfies the first three: AND / OR, 3 of 5, one row, and an AND chain with
    an attribute the key lacks"""
    chain = lf.and_chain_policy(3)
    return [lf.and_or_policy(), lf.threshold_policy(3, 5), ([[1]], [500]), chain], [11, 22, 201, 203, 204, 500, 100, 102, 999]


def at_size_policies(n, every=64):
    """n policies of 16 rows cycling through four shapes — an AND chain of 16, 8 of 16, (8 and) or (8 and), an AND chain of 5 padded
    up — and the key's attributes; every `every`-th policy (j % every == every - 1) is one the key does not satisfy"""
    chain16, thr, andor, chain5 = lf.and_chain_policy(16), lf.threshold_policy(8, 16), and_or_16(), lf.and_chain_policy(5)
    shapes = [chain16, thr, andor, (chain5[0], [600 + i for i in range(5)])]
    key = chain16[1] + thr[1][3:12] + andor[1][8:] + [600 + i for i in range(5)]          # 9 of the 16 Shamir rows, the second AND branch
    bad = ([[1, 1], [0, -1]], [700, 701])                                                  # needs 700 and 701: the key has neither
    return [bad if j % every == every - 1 else shapes[j % 4] for j in range(n)], key
