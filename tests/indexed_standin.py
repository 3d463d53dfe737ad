"""Stand-in engine of the Waters11 / LW11 Encrypt and BSW07 tables plan tests: the engine's function names on the oracle (host arrays
only; tensors are taken and given back as CPU tensors), with FixedBase.indexed as one oracle scalar multiplication per term and the
oracle's sum per output, fr_lsss_shares in Python integers, gt_multi_exp as gt_exp per factor and gt_mul per segment."""
import numpy as np

import bn254_py as o
from share_standin import ShareEngine
from sw05_fixture import kbytes, kints
from waters11_fixture import OracleEngineW11

R = o.R
NONE = 0xFFFFFFFF


def _host(x):
    return x.numpy() if type(x).__module__.startswith("torch") else x


class StandInFixedBase:
    def __init__(self, oracle, bases, g2=False):
        self.o, self.g2, self.width = oracle, bool(g2), 128 if g2 else 64
        self.bases = np.array(_host(bases), dtype=np.uint8, copy=True).reshape(-1, self.width)
        self.nbase, self.closed, self.calls = len(self.bases), False, 0

    def indexed(self, index, scalars, terms=None, out=None):
        assert not self.closed and out is None
        tensor = type(scalars).__module__.startswith("torch")
        if tensor:
            import torch
            assert isinstance(index, torch.Tensor) and index.dtype == torch.int32, "a device index is int32 / uint32"
            index = index.numpy().view(np.uint32)
        else:
            assert isinstance(index, np.ndarray) and index.dtype == np.uint32
        ks = kints(_host(scalars))
        index = np.asarray(index).reshape(-1, terms)
        n, P = len(ks) // terms, len(index)
        assert len(ks) == n * terms and 1 <= P <= n
        self.calls += 1
        mul, add = (self.o.g2_scalar_mul, self.o.g2_sum) if self.g2 else (self.o.g1_scalar_mul, self.o.g1_sum)
        res, ok = np.zeros((n, self.width), dtype=np.uint8), np.ones(n, dtype=np.uint8)
        sel, kk, owner = [], [], []
        for i in range(n):
            row = [int(v) for v in index[i % P]]
            if any(v != NONE and v >= self.nbase for v in row):
                ok[i] = 0
                continue
            for t, j in enumerate(row):
                if j != NONE and self.bases[j].any() and ks[i * terms + t] % R:
                    sel.append(j); kk.append(ks[i * terms + t]); owner.append(i)
        if sel:
            pts = np.asarray(mul(self.bases[sel].reshape(-1), kbytes(kk), threads=4)).reshape(-1, self.width)
            owner = np.array(owner)
            for i in np.unique(owner):
                res[i] = np.asarray(add(pts[owner == i].reshape(-1))).reshape(self.width)
        if tensor:
            return torch.from_numpy(res), torch.from_numpy(ok)
        return res, ok

    def close(self):
        self.closed = True


class IndexedEngine(ShareEngine, OracleEngineW11):
    """ShareEngine (ShareTree, the generator multiplications, g2_add) + OracleEngineW11 (g1_add, fr_lsss_weights) + the new entries"""

    def __init__(self, oracle):
        super().__init__(oracle)
        self.tables = []

    def FixedBase(self, bases, g2=False):
        self.tables.append(StandInFixedBase(self.o, bases, g2))
        return self.tables[-1]

    def generators(self):
        return np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8), np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)

    def fr_lsss_shares(self, matrix, vectors, rows=None, cols=None, out=None):
        M = np.asarray(kints(matrix), dtype=object).reshape(-1, rows, cols)
        V = np.asarray(kints(vectors), dtype=object).reshape(-1, cols)
        assert len(M) in (1, len(V))
        return kbytes([sum(int(a) * int(b) for a, b in zip(M[j if len(M) > 1 else 0][x], V[j])) for j in range(len(V)) for x in range(rows)]).reshape(len(V), rows, 32)

    def gt_multi_exp(self, x, k, seg_off):
        seg = [int(v) for v in seg_off]
        x = np.asarray(x, dtype=np.uint8).reshape(-1, 384)
        ks = [int(v) for v in k] if isinstance(k, (list, tuple)) else kints(k)
        if len(ks) != len(x):                                                  # one exponent list for every segment
            ks = [ks[i - a] for a, b in zip(seg, seg[1:]) for i in range(a, b)]
        p = np.asarray(self.o.gt_exp(x.reshape(-1), kbytes(ks))).reshape(-1, 384)
        out = []
        for a, b in zip(seg, seg[1:]):
            acc = np.frombuffer(o.gt_to_bytes(o.F12_ONE), dtype=np.uint8)
            for i in range(a, b):
                acc = np.asarray(self.o.gt_mul(acc, p[i])).reshape(384)
            out.append(acc)
        return np.stack(out) if out else np.zeros((0, 384), dtype=np.uint8)
