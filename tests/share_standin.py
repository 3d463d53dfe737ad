"""Stand-in engine of the BSW07 Encrypt and SW05 KeyGenerate plan tests: the engine's function names on the oracle (host arrays only),
with ShareTree and fr_poly_eval as the Python-integer restatement of tests/share_cases.py and the other fr_* in Python integers."""
import numpy as np

import bn254_py as o
import share_cases as sc
from sw05_fixture import OracleEngine, kbytes, kints
from gopairingbasedcryptography_amd import bsw07

R = o.R
G1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
G2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)


def tree_of(nodes):
    """the Leaf / Threshold tree of a node list [(parent, threshold)]"""
    built = [bsw07.Leaf(i) if not t else bsw07.Threshold.__new__(bsw07.Threshold) for i, (_, t) in enumerate(nodes)]
    for node, (_, t) in zip(built, nodes):
        if t:
            node.k, node.children = t, []
    for i, (parent, _) in enumerate(nodes):
        if i:
            built[parent].children.append(built[i])
    return built[0]


class StandInTree:
    def __init__(self, nodes):
        nodes = [(int(p), int(t)) for p, t in np.asarray(nodes, dtype=np.int64).reshape(-1, 2).tolist()]
        assert sc.preorder(tree_of(nodes)) == nodes, "the node list is not in depth-first preorder"
        self.tree = tree_of(nodes)
        self.leaves, self.coeffs, self.closed = sum(1 for _, t in nodes if not t), sc.n_coeffs(self.tree), False

    def share(self, secrets, coeffs=None):
        assert not self.closed
        tensor = type(secrets).__module__.startswith("torch")                 # tensors in, a (CPU) tensor out: the engine's behaviour
        if tensor:
            import torch
            secrets, coeffs = secrets.numpy(), None if coeffs is None else coeffs.numpy()
        s, q = kints(secrets), kints(coeffs) if coeffs is not None else []
        assert len(q) == len(s) * self.coeffs
        out = [v for j, sj in enumerate(s) for v in sc.share(self.tree, sj, q[j * self.coeffs:(j + 1) * self.coeffs])]
        res = kbytes(out).reshape(len(s), self.leaves, 32)
        return torch.from_numpy(res.copy()) if tensor else res

    def close(self):
        self.closed = True


class ShareEngine(OracleEngine):
    ShareTree = StandInTree

    def g2_sum(self, p): return self.o.g2_sum(p)
    def g1_scalar_mul_base(self, k): return self.o.g1_scalar_mul(G1, self._k(k), threads=4)
    def g2_scalar_mul_base(self, k): return self.o.g2_scalar_mul(G2, self._k(k), threads=4)
    def fr_inverse(self, a): return kbytes([pow(v, -1, R) if v % R else 0 for v in kints(a)]).reshape(-1, 32)

    def g2_add(self, a, b):
        a, b = np.asarray(a, dtype=np.uint8).reshape(-1, 128), np.asarray(b, dtype=np.uint8).reshape(-1, 128)
        return np.stack([np.asarray(self.o.g2_sum(np.concatenate([x, y]))).reshape(128) for x, y in zip(a, b)])

    def fr_poly_eval(self, coeffs, points, d=None, m=None):
        C, P = np.asarray(kints(coeffs), dtype=object).reshape(-1, d), np.asarray(kints(points), dtype=object).reshape(-1, m)
        k = max(len(C), len(P))
        pick = lambda a, j: a[j if len(a) > 1 else 0]
        return kbytes([sc.horner(list(pick(C, j)), x) for j in range(k) for x in pick(P, j)]).reshape(k, m, 32)
