"""Test helper: a seeded Gentry 2006 IBE instance (ibe/gentry06_ibe/gentry06_ibe.go, ibe/gentry06_cpa_ibe) from known secrets.  SetUp
restated on exponents: alpha and the logarithms eta_j of h_j = [eta_j] g2 are known scalars, so with e = e(g1, g2) every expected key
and ciphertext component is ONE multiplication of a generator (or one power of e) by the exponent the reference's sequence arrives at

    hid_j = [(eta_j - r_j) / (alpha - ID)] g2      u = [s (alpha - ID)] g1      v = e^s      w = e^(m - s eta_1)
    beta = SHA-256(u.Bytes() || v.Bytes() || w.Bytes()) mod r  (hashlib over the oracle's encodings)      y = e^(s eta_2 + s beta eta_3)

computed with oracle calls and hashlib alone: a route that shares nothing with the planner's sequence of engine calls.

Also here: the reference's own sequences of KeyGenerate / Encrypt / Decrypt written out with oracle calls, one identity at a time.  The
stand-in engine the plan test runs the planner on is tests/standin_engine.py (its hash_g1_gt_gt_to_fr is beta_rows, the hashlib restatement)."""
import hashlib

import numpy as np

import bn254_py as o
from sw05_fixture import kbytes, kints

R = o.R
G1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
G2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)


def sc(tag, i=0):
    return o.bench_scalar("gentry06-" + tag, i)


def transcript(u, v, w):
    """the 800 bytes h() hashes: G1Affine.Bytes() and twice GT.Bytes(), from in-memory structs, through the oracle's encoders"""
    return (o.g1_marshal(o.g1_from_bytes(bytes(u)), compressed=True) + o.gt_marshal(o.gt_from_bytes(bytes(v))) + o.gt_marshal(o.gt_from_bytes(bytes(w))))


def beta_of(u, v, w):
    """h(u, v, w) as a Python integer: fr.SetBytes(SHA-256(...)) reads the digest big-endian and reduces it"""
    return int.from_bytes(hashlib.sha256(transcript(np.asarray(u).tobytes(), np.asarray(v).tobytes(), np.asarray(w).tobytes())).digest(), "big") % R


def beta_rows(u, v, w):
    u, v, w = (np.asarray(x, dtype=np.uint8).reshape(-1, width) for x, width in ((u, 64), (v, 384), (w, 384)))
    return kbytes([beta_of(a, b, c) for a, b, c in zip(u, v, w)]).reshape(-1, 32).copy()


class Instance:
    """n identities under k public points (1: gentry06_cpa_ibe, 3: gentry06_ibe); identity `alpha_at` (if any) equals alpha"""

    def __init__(self, oracle, n, k, tag="", alpha_at=None):
        self.oracle, self.n, self.k, self.alpha_at = oracle, n, k, alpha_at
        tag += "k%d-" % k
        g1mul = lambda ks: np.asarray(oracle.g1_scalar_mul(G1, kbytes(ks), threads=8)).reshape(-1, 64)
        g2mul = lambda ks: np.asarray(oracle.g2_scalar_mul(G2, kbytes(ks), threads=8)).reshape(-1, 128)
        epow = lambda ks: np.asarray(oracle.gt_exp(np.tile(self.e, (len(ks), 1)), kbytes(ks), threads=8)).reshape(-1, 384)
        self.alpha, self.eta = sc(tag + "alpha"), [sc(tag + "eta", j) for j in range(k)]
        self.ids = [self.alpha if i == alpha_at else sc(tag + "id", i) for i in range(n)]
        self.r = [[sc(tag + "r", i * k + j) for j in range(k)] for i in range(n)]
        self.s, self.msg = ([sc(tag + name, i) for i in range(n)] for name in ("s", "msg"))
        self.g1_alpha, self.h = g1mul([self.alpha])[0], g2mul(self.eta)
        self.e = np.asarray(oracle.pair_batch(G1, G2)).reshape(384)
        self.e_gh = epow(self.eta)
        self.messages = epow(self.msg)
        # the expected outputs, on exponents
        self.ok = np.array([i != alpha_at for i in range(n)], dtype=np.uint8)
        inv = [pow((self.alpha - ID) % R, -1, R) if good else 0 for ID, good in zip(self.ids, self.ok)]
        self.hids = g2mul([(self.eta[j] - self.r[i][j]) * inv[i] for i in range(n) for j in range(k)]).reshape(n, k, 128)
        self.rids = kbytes([self.r[i][j] * int(self.ok[i]) for i in range(n) for j in range(k)]).reshape(n, k, 32).copy()
        self.u = g1mul([s * (self.alpha - ID) for s, ID in zip(self.s, self.ids)])
        self.v = epow(self.s)
        self.w = epow([m - s * self.eta[0] for m, s in zip(self.msg, self.s)])
        if k == 3:
            self.beta = [beta_of(*uvw) for uvw in zip(self.u, self.v, self.w)]
            self.y = epow([s * self.eta[1] + s * b * self.eta[2] for s, b in zip(self.s, self.beta)])

    def ct(self, rows=None):
        """(u, v, w[, y]) of the given rows (all by default), copies"""
        rows = list(range(self.n)) if rows is None else list(rows)
        return tuple(np.array(x[rows], copy=True) for x in ((self.u, self.v, self.w) + ((self.y,) if self.k == 3 else ())))

    def valid(self):
        return [i for i in range(self.n) if i != self.alpha_at]

    # ---- the reference's sequences, one identity at a time (every line an oracle call or Python integers mod r)
    def reference_keygen(self, i):
        """KeyGenerate :145-180; None where the reference returns its error"""
        a = (self.alpha - self.ids[i]) % R
        inv = pow(a, -1, R) if a else 0                                       # fr.Element.Inverse: 0 -> 0
        if inv == 0:
            return None
        hids = []
        for j in range(self.k):
            g2_inv_rid = self.oracle.g2_scalar_mul(G2, kbytes([-self.r[i][j]]))[0]
            h_add = self.oracle.g2_sum(np.stack([self.h[j], g2_inv_rid]))
            hids.append(self.oracle.g2_scalar_mul(h_add, kbytes([inv]))[0])
        return kbytes(self.r[i]).reshape(self.k, 32), np.stack(hids)

    def reference_encrypt(self, i):
        """Encrypt :192-245, the pairings recomputed as the reference recomputes them"""
        orc, s, ID = self.oracle, self.s[i], self.ids[i]
        g1_alpha_s = orc.g1_scalar_mul(self.g1_alpha, kbytes([s]))[0]
        g1_neg_s_id = orc.g1_scalar_mul(G1, kbytes([-(s * ID)]))[0]
        u = np.asarray(orc.g1_sum(np.stack([g1_alpha_s, g1_neg_s_id]))).reshape(64)
        v = orc.gt_exp(orc.pair_batch(G1, G2)[0], kbytes([s]))[0]
        w = orc.gt_mul(orc.gt_exp(orc.pair_batch(G1, self.h[0])[0], kbytes([-s]))[0], self.messages[i])[0]
        if self.k == 1:
            return u, v, w
        beta = beta_of(u, v, w)
        e2 = orc.gt_exp(orc.pair_batch(G1, self.h[1])[0], kbytes([s]))[0]
        e3 = orc.gt_exp(orc.pair_batch(G1, self.h[2])[0], kbytes([s * beta]))[0]
        return u, v, w, orc.gt_mul(e2, e3)[0]

    def reference_decrypt(self, rids, hids, u, v, w, y=None):
        """Decrypt :264-314 (gentry06_cpa_ibe: the recovery alone); None where the check fails"""
        orc, r = self.oracle, kints(rids)
        if self.k == 3:
            beta = beta_of(u, v, w)
            v_exp = orc.gt_exp(v, kbytes([r[1] + r[2] * beta]))[0]
            hq = orc.g2_sum(np.stack([hids[1], orc.g2_scalar_mul(hids[2], kbytes([beta]))[0]]))
            y_prime = orc.gt_mul(v_exp, orc.pair_batch(u, hq)[0])[0]
            if np.asarray(y_prime).tobytes() != np.asarray(y).tobytes():
                return None
        m = orc.gt_mul(w, orc.pair_batch(u, hids[0])[0])[0]
        return orc.gt_mul(m, orc.gt_exp(v, kbytes([r[0]]))[0])[0]


def tamper(inst, oracle, how, rows):
    """(ciphertext, the rows it spoils): a copy of the ciphertexts of `rows` with y replaced by y e ("y", first row), w of the first two
    rows swapped ("w"), or u of the first row negated ("u")"""
    u, v, w, y = inst.ct(rows)
    if how == "y":
        y[0] = oracle.gt_mul(y[0], inst.e)[0]
        return (u, v, w, y), [0]
    if how == "w":
        w[[0, 1]] = w[[1, 0]]
        return (u, v, w, y), [0, 1]
    u[0] = np.frombuffer(o.g1_to_bytes(o.g1_neg(o.g1_from_bytes(u[0].tobytes()))), dtype=np.uint8)
    return (u, v, w, y), [0]
