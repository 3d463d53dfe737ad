"""Test helper: a seeded Waters 2005 IBE instance (ibe/waters05_ibe/waters05_ibe.go) from known secrets.  SetUp restated on exponents:
alpha, u' and u_0 .. u_255 are known scalars, every public point is ONE multiplication of a generator by the oracle, so the expected
outputs of KeyGenerate and Encrypt are single generator multiplications too (the Waters hash of an identity has the known logarithm
h = u' + sum_{Id[i] = 1} u_i): a route that shares nothing with the table sums under test.

Also here: the reference's own sequence of operations written out with oracle calls (the chain of G2Affine.Add over Id[], the scalar
multiplication, Pair / Mul / Div of Decrypt).  The stand-in engine the plan test runs the planner on is tests/standin_engine.py."""
import hashlib

import numpy as np

import bn254_py as o
from sw05_fixture import kbytes

R = o.R
G1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
G2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)


def sc(tag, i=0):
    return o.bench_scalar("waters05-" + tag, i)


def id_bits(s):
    """Id[] of NewWaters05IBEIdentity: byte by byte, bit 7 first"""
    return [(b >> (7 - t)) & 1 for b in hashlib.sha256(s.encode()).digest() for t in range(8)]


class Instance:
    def __init__(self, oracle, ids, tag=""):
        self.oracle, self.ids, n = oracle, list(ids), len(ids)
        g1mul = lambda ks: np.asarray(oracle.g1_scalar_mul(G1, kbytes(ks), threads=8)).reshape(-1, 64)
        g2mul = lambda ks: np.asarray(oracle.g2_scalar_mul(G2, kbytes(ks), threads=8)).reshape(-1, 128)
        self.alpha, self.u_prime_k, self.u_k = sc(tag + "alpha"), sc(tag + "u'"), [sc(tag + "u", i) for i in range(256)]
        self.g2_alpha, self.g1_alpha = g2mul([self.alpha])[0], g1mul([self.alpha])[0]
        self.u_prime, self.ui = g2mul([self.u_prime_k])[0], g2mul(self.u_k)
        self.e = np.asarray(oracle.pair_batch(G1, G2)).reshape(384)
        self.e_alpha = np.asarray(oracle.pair_batch(self.g1_alpha, G2)).reshape(384)
        self.bits = [id_bits(s) for s in self.ids]
        self.h = [(self.u_prime_k + sum(u for u, b in zip(self.u_k, bits) if b)) % R for bits in self.bits]       # log_g2 H(id)
        self.r, self.t, self.msg = ([sc(tag + name, i) for i in range(n)] for name in ("r", "t", "msg"))
        self.messages = np.asarray(oracle.gt_exp(np.tile(self.e, (n, 1)), kbytes(self.msg), threads=8)).reshape(n, 384)
        # the expected outputs, on exponents
        self.d1 = g2mul([(self.alpha + r * h) % R for r, h in zip(self.r, self.h)])
        self.d2 = g1mul(self.r)
        self.c1 = np.asarray(oracle.gt_exp(np.tile(self.e, (n, 1)), kbytes([(m + self.alpha * t) % R for m, t in zip(self.msg, self.t)]), threads=8)).reshape(n, 384)
        self.c2 = g1mul(self.t)
        self.c3 = g2mul([t * h % R for t, h in zip(self.t, self.h)])

    def rows(self, ks):
        return kbytes(ks).reshape(-1, 32).copy()

    # ---- the reference's sequence, one identity at a time
    def reference_hash(self, j):
        """product = U'; for i: if Id[i] == 1: product.Add(&product, &ui[i])"""
        product = self.u_prime
        for i, b in enumerate(self.bits[j]):
            if b:
                product = self.oracle.g2_sum(np.stack([product, self.ui[i]]))
        return product

    def reference_keygen(self, j):
        product = self.oracle.g2_scalar_mul(self.reference_hash(j), kbytes([self.r[j]]))[0]
        return self.oracle.g2_sum(np.stack([self.g2_alpha, product])), self.oracle.g1_scalar_mul(G1, kbytes([self.r[j]]))[0]

    def reference_encrypt(self, j):
        e_t = self.oracle.gt_exp(self.oracle.pair_batch(self.g1_alpha, G2)[0], kbytes([self.t[j]]))[0]
        return (self.oracle.gt_mul(e_t, self.messages[j])[0], self.oracle.g1_scalar_mul(G1, kbytes([self.t[j]]))[0],
                self.oracle.g2_scalar_mul(self.reference_hash(j), kbytes([self.t[j]]))[0])

    def reference_decrypt(self, d1, d2, c1, c2, c3):
        m = self.oracle.gt_mul(c1, self.oracle.pair_batch(d2, c3)[0])[0]
        return self.oracle.gt_div(m, self.oracle.pair_batch(c2, d1)[0])[0]
