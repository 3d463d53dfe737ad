"""Cases and expectations of the AFP25 scheme tests (tests/test_afp25_scheme_plan.py on the stand-in engine, tests/test_afp25_scheme_gpu.py
on the GPU).  Every expectation is the scheme's equation restated in SCALARS from the known secrets and evaluated with the oracle — one
multiplication of a generator per group element, one pairing and one power per GT element, bn254_py.hash_to_g1 for h(t) — and none comes
from the planner or from any engine route:

    G1ExpTauPowers[i] = [tau^(i+1) mod r] g1 (Python pow)      G2ExpTau = [tau] g2      G2ExpMsk = [msk] g2
    C1[0] = [r1 + r2 msk] g2      C1[1] = [r1 (id - tau)] g2      C1[2] = [-r2] g2      C2 = M e(h(t), g2)^(-r2 msk)
    D = [prod (tau - id)] g1      sk = [msk](D + h(t)) by the oracle's addition and multiplication

Shapes, the smallest at which each stage can still go wrong: B = 4 with batches of 1, 3 and 4 identities and a label per batch, the labels
0, 5 and 70 bytes long (70 crosses a SHA-256 block); one batch of B = 65 (66 table bases: the fused openings cross a wavefront); B = 1.
The B = 4 case carries the special items: id = 0 ([id]_2 is infinity), id = tau (C1[1] is the point at infinity), id = r - 1, r1 = 0,
r2 = 0 (C1[2] is infinity and C2 = M).  A case is built once per process and shared."""
import functools

import numpy as np

import bn254_py as o
from sw05_fixture import kbytes

R = o.R
DST = b"Hash Bytes To Element In G1"                                          # hash.BytesToG1's tag
G1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
G2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
LABELS = (b"", b"batch", bytes(range(70)))
SHAPES = {"b4": (4, (1, 3, 4)), "b65": (65, (65,)), "b1": (1, (1,))}


def sc(tag, i=0):
    return o.bench_scalar("afp25-scheme-" + tag, i)


class Case:
    def __init__(self, orc, name):
        self.name, self.orc = name, orc
        self.B, self.counts = SHAPES[name]
        self.counts = list(self.counts)
        self.n, self.k = sum(self.counts), len(self.counts)
        self.tau, self.msk = sc(name + "tau"), sc(name + "msk")
        self.labels = list(LABELS[:self.k])
        self.label_of = np.repeat(np.arange(self.k), self.counts)
        self.ids = [sc(name + "id", i) for i in range(self.n)]
        self.r1 = [sc(name + "r1", i) for i in range(self.n)]
        self.r2 = [sc(name + "r2", i) for i in range(self.n)]
        if name == "b4":                                                       # batch 1 = items 1 .. 3, batch 2 = items 4 .. 7
            self.ids[1], self.ids[2], self.ids[3] = 0, self.tau, R - 1
            self.r1[5], self.r2[6] = 0, 0
        self.msg = [sc(name + "msg", i) for i in range(self.n)]
        self.batches = [self.ids[sum(self.counts[:j]):sum(self.counts[:j + 1])] for j in range(self.k)]

    # ---- the expectations, each computed once
    def _g1(self, ks): return np.asarray(self.orc.g1_scalar_mul(G1, kbytes(ks), threads=4)).reshape(-1, 64)
    def _g2(self, ks): return np.asarray(self.orc.g2_scalar_mul(G2, kbytes(ks), threads=4)).reshape(-1, 128)

    @functools.cached_property
    def e(self):
        return np.asarray(self.orc.pair_batch(G1, G2)).reshape(1, 384)

    @functools.cached_property
    def messages(self):
        return np.asarray(self.orc.gt_exp(np.tile(self.e, (self.n, 1)), kbytes(self.msg))).reshape(self.n, 384)

    @functools.cached_property
    def mpk(self):
        in_g2 = self._g2([self.tau, self.msk])
        return {"G1ExpTauPowers": self._g1([pow(self.tau, i + 1, R) for i in range(self.B)]), "G2ExpTau": in_g2[0], "G2ExpMsk": in_g2[1]}

    @functools.cached_property
    def points(self):
        return np.stack([np.frombuffer(o.g1_to_bytes(o.hash_to_g1(t, DST)), dtype=np.uint8) for t in self.labels])

    @functools.cached_property
    def C1(self):
        cols = ([(a + b * self.msk) % R for a, b in zip(self.r1, self.r2)], [a * (i - self.tau) % R for a, i in zip(self.r1, self.ids)], [-b % R for b in self.r2])
        return np.stack([self._g2(c) for c in cols], 1)                        # [n, 3, 128]

    @functools.cached_property
    def C2(self):
        e_h = np.asarray(self.orc.pair_batch(self.points, np.tile(G2, (self.k, 1)))).reshape(self.k, 384)[self.label_of]
        blind = self.orc.gt_exp(e_h, kbytes([-b * self.msk % R for b in self.r2]))
        return np.asarray(self.orc.gt_mul(blind, self.messages)).reshape(self.n, 384)

    @functools.cached_property
    def D(self):
        f_tau = []
        for batch in self.batches:
            v = 1
            for i in batch:
                v = v * (self.tau - i) % R
            f_tau.append(v)
        return self._g1(f_tau)

    @functools.cached_property
    def sk(self):
        sums = np.stack([np.asarray(self.orc.g1_sum(np.stack([d, h]))).reshape(64) for d, h in zip(self.D, self.points)])
        return np.stack([np.asarray(self.orc.g1_scalar_mul(s, kbytes([self.msk]))).reshape(64) for s in sums])


_cases = {}


def case(orc, name):
    if name not in _cases:
        _cases[name] = Case(orc, name)
    return _cases[name]
