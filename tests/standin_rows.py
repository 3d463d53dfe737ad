"""The stand-in engine of tests/standin_gtfixed.py with g1 / g2_scalar_mul in their ROW form (nbase bases for nbase * m scalars, row-major:
the bases expanded per scalar for the oracle, which knows one base or one base per scalar only) and fr_random from the Python oracle of
tests/chacha_cases.py, every draw written down as (n, stream, first).  Nothing here shares code with rows29.hip.hpp or with the planners'
sequence of calls."""
import numpy as np

import chacha_cases as cc
from standin_engine import _rows
from standin_gtfixed import GTFixedStandIn


class RowsStandIn(GTFixedStandIn):
    def __init__(self, oracle, without=()):
        super().__init__(oracle, without)
        self.draws = []

    def _row_mul(self, mul, width, b, k):
        b, k = _rows(b, width), np.asarray(self._k(k), dtype=np.uint8).reshape(-1, 32)
        if len(b) not in (1, len(k)):
            if not 1 < len(b) < len(k) or len(k) % len(b):
                raise ValueError("need one base, one base per scalar, or one base per row of n / nbase scalars")
            b = np.repeat(b, len(k) // len(b), axis=0)
        return mul(b.reshape(-1), k.reshape(-1), threads=4)

    def g1_scalar_mul(self, b, k): return self._row_mul(self.o.g1_scalar_mul, 64, b, k)
    def g2_scalar_mul(self, b, k): return self._row_mul(self.o.g2_scalar_mul, 128, b, k)

    def fr_random(self, seed, n, stream=0, first=0, out=None, like=None):
        self.draws.append((n, stream, first))
        return cc.scalars(bytes(seed), stream, first, n)
