"""The stand-in engine of tests/standin_engine.py with bn254.ShareForest added: a StandInTree per tree, an item at a time — ShareSecret as
tests/share_cases.py restates it and bsw07.decrypt_plan, both in Python integers — with the padding the real handle promises (columns
>= L_t zero, coefficients beyond C_t and held bytes beyond L_t never looked at, a tree id of T or more an all-zero row and ok = 0).
Nothing here shares code with forest29.hip.hpp or with the planners' sequence of calls."""
import numpy as np

from standin_engine import StandInEngine, StandInTree, _is_tensor, _rows, on_arrays


class StandInForest:
    def __init__(self, node_lists):
        self.each = [StandInTree(nodes) for nodes in node_lists]
        self.trees, self.tree_leaves, self.tree_coeffs = len(self.each), [t.leaves for t in self.each], [t.coeffs for t in self.each]
        self.leaves, self.coeffs, self.closed, self.calls = max(self.tree_leaves), max(self.tree_coeffs), False, []

    def _ids(self, tree_of):
        if _is_tensor(tree_of):
            assert str(tree_of.dtype) == "torch.int32", "device tree ids are int32"
        else:
            assert isinstance(tree_of, np.ndarray) and tree_of.dtype == np.uint32, "host tree ids are a uint32 array"

    def share(self, tree_of, secrets, coeffs=None):
        assert not self.closed
        self._ids(tree_of)
        self.calls.append("share")
        return on_arrays(self._share, tree_of, secrets, coeffs)

    def _share(self, tree_of, secrets, coeffs):
        ids, s = np.asarray(tree_of).view(np.uint32).reshape(-1), _rows(secrets, 32)
        assert len(ids) == len(s)
        q = _rows(coeffs, 32).reshape(len(s), self.coeffs, 32) if self.coeffs else None
        out, ok = np.zeros((len(s), self.leaves, 32), dtype=np.uint8), np.zeros(len(s), dtype=np.uint8)
        for i, t in enumerate(int(v) for v in ids):
            if t < self.trees:
                tr = self.each[t]
                out[i, :tr.leaves] = tr._share(s[i], q[i, :tr.coeffs] if tr.coeffs else None)[0]
                ok[i] = 1
        return out, ok

    def weights(self, tree_of, held):
        assert not self.closed
        self._ids(tree_of)
        self.calls.append("weights")
        return on_arrays(self._weights, tree_of, held)

    def _weights(self, tree_of, held):
        ids, h = np.asarray(tree_of).view(np.uint32).reshape(-1), _rows(held, self.leaves)
        assert len(ids) == len(h)
        w, ok = np.zeros((len(h), self.leaves, 32), dtype=np.uint8), np.zeros(len(h), dtype=np.uint8)
        for i, t in enumerate(int(v) for v in ids):
            if t < self.trees:
                tr = self.each[t]
                wi, oki = tr._weights(h[i, :tr.leaves])
                w[i, :tr.leaves], ok[i] = wi[0], oki[0]
        return w, ok

    def close(self):
        self.closed = True


class ForestStandIn(StandInEngine):
    def __init__(self, oracle, without=()):
        super().__init__(oracle, without)
        self.forests = []

    def ShareForest(self, node_lists):
        self.forests.append(StandInForest(node_lists))
        return self.forests[-1]
