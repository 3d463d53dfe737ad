"""A Boneh-Franklin BasicIdent instance for the plan and GPU tests of bf01.py: n identities, n byte messages whose lengths cycle
through 0, 5, 32, 100, 400, and the expected KeyGenerate / Encrypt / Decrypt outputs computed by the oracle IN THE REFERENCE'S ORDER
(ibe/bf01_ibe/bf01_ibe.go): Q_id = hash.ToG2(id) (the Python oracle's hash_to_g2), sk = [x] Q_id, C1 = [r] g1,
gid = GT.Exp(Pair(g1x, Q_id), r) — pair, THEN the exponentiation in GT, then GT.Bytes() — C2 = Xor(M, bytes), and Decrypt's
gid = Pair(C1, sk).  Nothing here calls the planner."""
import hashlib

import numpy as np

import bn254_py as o
import mask_cases as mc
from sw05_fixture import kbytes

R = o.R
DST = b"Hash String To Element In G2"
LENGTHS = [0, 5, 32, 100, 400]
NAMES = ["alice@example.com", "bob", b"carol\x00bytes", "däve", ""]
G1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)


def _scalar(tag, i):
    return int.from_bytes(hashlib.sha256(("bf01/%s/%d" % (tag, i)).encode()).digest() * 2, "big") % R


def flat_messages(msgs):
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    data = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()
    return data, off


class Instance:
    def __init__(self, oracle, n, r=None):
        self.n, self.x = n, _scalar("x", 0)
        self.ids = [NAMES[i % len(NAMES)] if i < len(NAMES) else "user-%d@example.org" % i for i in range(n)]
        self.id_bytes = [i.encode("utf-8") if isinstance(i, str) else i for i in self.ids]
        self.msgs = [hashlib.shake_256(b"bf01 message %d" % i).digest(LENGTHS[i % len(LENGTHS)]) for i in range(n)]
        self.r = [_scalar("r", i) for i in range(n)] if r is None else list(r)
        self.data, self.off = flat_messages(self.msgs)
        # the reference, step by step
        self.qids = np.stack([np.frombuffer(o.g2_to_bytes(o.hash_to_g2(b, DST)), dtype=np.uint8) for b in self.id_bytes])
        self.g1x = np.asarray(oracle.g1_scalar_mul(G1, kbytes([self.x]))).reshape(64)
        self.sk = np.asarray(oracle.g2_scalar_mul(self.qids.reshape(-1), kbytes([self.x] * n), threads=4)).reshape(n, 128)
        self.c1 = np.asarray(oracle.g1_scalar_mul(G1, kbytes(self.r), threads=4)).reshape(n, 64)
        e = oracle.pair_batch(np.tile(self.g1x, n), self.qids.reshape(-1), threads=4)             # Pair(g1x, Q_id) ...
        self.gid = np.asarray(oracle.gt_exp(e, kbytes(self.r), threads=4)).reshape(n, 384)        # ... then GT.Exp(., r)
        self.masks = [mc.mask_of(g) for g in self.gid]
        cut = [mc.xor_cut(m, k) for m, k in zip(self.msgs, self.masks)]
        self.c2 = [c for c, _ in cut]                                                             # zero-extended to the message's length
        self.c2_len = np.array([L for _, L in cut], dtype=np.uint32)
        self.c2_data = np.frombuffer(b"".join(self.c2), dtype=np.uint8).copy()
        gid_dec = np.asarray(oracle.pair_batch(self.c1.reshape(-1), self.sk.reshape(-1), threads=4)).reshape(n, 384)
        self.dec = [mc.xor_cut(c, mc.mask_of(g))[0] for c, g in zip(self.c2, gid_dec)]           # Decrypt on the buffer as it stands
        self.dec_data = np.frombuffer(b"".join(self.dec), dtype=np.uint8).copy()

    def recovered(self):
        """what a round trip must give: message[:384], zeros to the message's length"""
        return [m[:384] + bytes(max(0, len(m) - 384)) for m in self.msgs]
