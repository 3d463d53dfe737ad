"""Instances of the three signature schemes for the plan and GPU tests of bls01.py, zss04.py and bb04sig.py: n messages under one key,
with keys and signatures computed by the oracle IN THE REFERENCE'S ORDER (signature/bls01_signature/bls_signature.go:38-69,
signature/zss04_signature/zss04_signature.go:178-257, signature/bb04_signature/bb04_signature.go:171-240): Python integers for
everything in Fr, one oracle scalar multiplication per key and per signature, the Python oracle's hash_to_g2.  Nothing here calls a
planner.  Each instance comes with an adapter (each / batch / values) that hands the planner's functions one uniform set of arrays:
key (a list of rows), msg (scalars or hashed points), sig (a list of arrays)."""
import hashlib

import numpy as np

import bn254_py as o
from sw05_fixture import kbytes
from gopairingbasedcryptography_amd import bb04sig, bls01, zss04

R = o.R
G1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
G2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
DST_BYTES_G2 = b"Hash Bytes To Element In G2"
LENGTHS = [0, 5, 32, 64, 65, 100]                      # ZSS04: at most 64 bytes go through fr_set_bytes64, longer ones through the host
SCHEMES = ("zss04", "bb04", "bls01")


def scalar(tag, i=0):
    return int.from_bytes(hashlib.sha256(("signatures/%s/%d" % (tag, i)).encode()).digest() * 2, "big") % R


def message(i):
    return hashlib.shake_256(b"signed message %d" % i).digest(LENGTHS[i % len(LENGTHS)])


def inverse(v):
    return pow(v % R, -1, R) if v % R else 0           # fr.Element.Inverse: 0 -> 0


def g1_mul(oracle, ks):
    return np.asarray(oracle.g1_scalar_mul(G1, kbytes(ks), threads=4)).reshape(-1, 64)


def g2_mul(oracle, ks):
    return np.asarray(oracle.g2_scalar_mul(G2, kbytes(ks), threads=4)).reshape(-1, 128)


_hashed = {}


def bytes_to_g2(m):
    if m not in _hashed:
        _hashed[m] = np.frombuffer(o.g2_to_bytes(o.hash_to_g2(m, DST_BYTES_G2)), dtype=np.uint8)
    return _hashed[m]


class Instance:
    """scheme, n, key / other_key (rows), msgs (bytes, or integers for bb04), msg (rows the planner takes), sig (list of arrays)"""

    def __init__(self, oracle, scheme, n, same=()):
        """same: pairs (i, j) — item j signs item i's message (with item i's r, for bb04)"""
        self.scheme, self.n, self.oracle = scheme, n, oracle
        self.eg = np.asarray(oracle.pair_batch(G1, G2)).reshape(384)
        src = list(range(n))
        for i, j in same:
            src[j] = i
        if scheme == "zss04":
            self.x, x2 = scalar("zss04/x"), scalar("zss04/x2")
            self.msgs = [message(s) for s in src]
            self.hm = [int.from_bytes(m, "big") % R for m in self.msgs]                       # hash.BytesToField: SetBytes of the raw message
            self.key, self.other_key = [g2_mul(oracle, [self.x])[0]], [g2_mul(oracle, [x2])[0]]
            self.msg = kbytes(self.hm).reshape(n, 32).copy()
            self.sig = [g1_mul(oracle, [inverse(h + self.x) for h in self.hm])]
        elif scheme == "bb04":
            self.alpha, self.beta = scalar("bb04/alpha"), scalar("bb04/beta")
            self.msgs = [scalar("bb04/m", s) for s in src]
            self.r = [scalar("bb04/r", s) for s in src]
            self.key = [g2_mul(oracle, [self.alpha])[0], g2_mul(oracle, [self.beta])[0]]
            self.other_key = [self.key[0], g2_mul(oracle, [scalar("bb04/beta2")])[0]]
            self.msg = kbytes(self.msgs).reshape(n, 32).copy()
            sigma = g1_mul(oracle, [inverse(self.alpha + r * self.beta + m) for m, r in zip(self.msgs, self.r)])
            self.sig = [kbytes(self.r).reshape(n, 32).copy(), sigma]
        else:
            self.x = scalar("bls01/x")
            self.msgs = [message(s) for s in src]
            self.key, self.other_key = [g1_mul(oracle, [self.x])[0]], [g1_mul(oracle, [scalar("bls01/x2")])[0]]
            self.msg = np.stack([bytes_to_g2(m) for m in self.msgs])
            self.sig = [np.asarray(oracle.g2_scalar_mul(self.msg.reshape(-1), kbytes([self.x] * n), threads=4)).reshape(n, 128)]

    # ---- the planner's functions on (key, msg, sig)
    def each(self, eng, key, msg, sig):
        if self.scheme == "zss04":
            return zss04.verify_each(eng, key[0], self.eg, sig[0], hm=msg)
        if self.scheme == "bb04":
            return bb04sig.verify_each(eng, key[0], key[1], self.eg, msg, sig[0], sig[1])
        return bls01.verify_each(eng, key[0], G1, sig[0], hashed=msg)

    def batch(self, eng, key, msg, sig, rho, group):
        if self.scheme == "zss04":
            return zss04.verify_batch(eng, key[0], self.eg, sig[0], rho, hm=msg, group=group)
        if self.scheme == "bb04":
            return bb04sig.verify_batch(eng, key[0], key[1], self.eg, msg, sig[0], sig[1], rho, group=group)
        return bls01.verify_batch(eng, key[0], G1, sig[0], rho, hashed=msg, group=group)

    def values(self, eng, key, msg, sig, rho, seg):
        """the group equation itself on host arrays"""
        rho = np.ascontiguousarray(rho).reshape(-1)
        if self.scheme == "zss04":
            return zss04.group_values(eng, key[0].reshape(1, 128), sig[0], msg, rho, seg)
        if self.scheme == "bb04":
            return bb04sig.group_values(eng, key[0].reshape(1, 128), key[1].reshape(1, 128), msg.reshape(-1), sig[0].reshape(-1), sig[1], rho, seg)
        return bls01.group_values(eng, key[0].reshape(1, 64), G1, sig[0], msg, rho, seg)

    def point_sig(self):
        """index into sig of the group element, and its row width"""
        return (1, 64) if self.scheme == "bb04" else (0, 128 if self.scheme == "bls01" else 64)

    def forged(self, positions):
        """sig with the group element at `positions` replaced by a valid signature of ANOTHER message (the next item's, cyclically)"""
        k, _ = self.point_sig()
        sig = [np.array(a, copy=True) for a in self.sig]
        for p in positions:
            sig[k][p] = self.sig[k][(p + 1) % self.n]
        return sig

    def tampered_msg(self, positions):
        msg = np.array(self.msg, copy=True)
        for p in positions:
            msg[p] = self.msg[(p + 1) % self.n]
        return msg
