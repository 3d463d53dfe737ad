"""The stand-in engine of tests/standin_member.py with the entries bb04sibe.py and bb04ibe.py call besides: GTFixedBase as one f12_pow per
term and one f12_mul per factor in Python integers (the scalar as the integer it is, an index >= nbase a zero row with ok = 0), and sha256
from hashlib.  Nothing here shares code with gtfixed29.hip.hpp or with the planners' sequence of calls."""
import hashlib

import numpy as np

import bn254_py as o
from standin_engine import INDEX_NONE, _is_tensor, on_arrays
from standin_member import MemberStandIn


class StandInGTFixedBase:
    """bn254.GTFixedBase in Python integers"""

    def __init__(self, bases):
        rows = np.array(bases.numpy() if _is_tensor(bases) else bases, dtype=np.uint8, copy=True).reshape(-1, 384)
        self.bases = [o.gt_from_bytes(r.tobytes()) for r in rows]
        self.nbase, self.closed, self.calls = len(rows), False, []

    def table_bytes(self):
        return self.nbase << 22

    def pow(self, scalars, base=0, out=None):
        assert 0 <= base < self.nbase and out is None
        index = np.array([base], dtype=np.uint32)
        if _is_tensor(scalars):
            import torch
            index = torch.from_numpy(index.view(np.int32))
        return self.indexed(index, scalars, terms=1)[0]

    def indexed(self, index, scalars, terms=None, out=None, ok_out=None):
        assert not self.closed and out is None and ok_out is None
        if _is_tensor(scalars):
            assert _is_tensor(index) and str(index.dtype) == "torch.int32", "a device index is int32 / uint32"
        else:
            assert isinstance(index, np.ndarray) and index.dtype == np.uint32
        return on_arrays(self._indexed, index, scalars, terms)

    def _indexed(self, index, scalars, terms):
        k = [int.from_bytes(r.tobytes(), "little") for r in np.asarray(scalars, dtype=np.uint8).reshape(-1, 32)]      # as they are: not reduced
        index = index.view(np.uint32).reshape(-1, terms)
        n, P = len(k) // terms, len(index)
        assert len(k) == n * terms and 1 <= P <= n
        self.calls.append((n, terms, P))
        res, ok = np.zeros((n, 384), dtype=np.uint8), np.ones(n, dtype=np.uint8)
        for i in range(n):
            row = [int(v) for v in index[i % P]]
            if any(v != INDEX_NONE and v >= self.nbase for v in row):
                ok[i] = 0
                continue
            acc = o.F12_ONE
            for t, j in enumerate(row):
                if j != INDEX_NONE:
                    acc = o.f12_mul(acc, o.f12_pow(self.bases[j], k[i * terms + t]))
            res[i] = np.frombuffer(o.gt_to_bytes(acc), dtype=np.uint8)
        return res, ok

    def close(self):
        self.closed = True


class GTFixedStandIn(MemberStandIn):
    def GTFixedBase(self, bases):
        return StandInGTFixedBase(bases)

    def sha256(self, msgs, msg_off=None):
        if msg_off is not None:
            buf = np.asarray(msgs, dtype=np.uint8).tobytes()
            msgs = [buf[int(a):int(b)] for a, b in zip(msg_off[:-1], msg_off[1:])]
        return np.frombuffer(b"".join(hashlib.sha256(bytes(m)).digest() for m in msgs), dtype=np.uint8).reshape(-1, 32).copy()
