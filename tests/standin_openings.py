"""The stand-in engine of tests/standin_gtfixed.py with the two new names gwww25.py and afp25.py call besides — fr_poly_from_roots_segments and
FixedBase.openings — and the older polynomial entries afp25.opening_proofs needs for comparison (fr_to_bytes, fr_poly_from_roots,
fr_poly_quotients), all in Python integers; fr_add broadcasts a single second operand as the engine's does.  An opening is one oracle scalar
multiplication per coefficient of the quotient and the oracle's sum; ok follows the reference's rule, counted: exactly one identity of the
batch equals it modulo r (with the caller's coefficient rows: the identity is a root of its row, and not twice).  Nothing here shares code
with openings29.hip.hpp or with the planners' sequence of calls."""
import numpy as np

import bn254_py as o
from standin_engine import StandInFixedBase, _pick, on_arrays
from standin_gtfixed import GTFixedStandIn
from sw05_fixture import kbytes, kints

R = o.R


def poly_from_roots(roots):
    c = [1]
    for root in roots:
        c = [((c[i - 1] if i else 0) - root * (c[i] if i < len(c) else 0)) % R for i in range(len(c) + 1)]
    return c


def quotient(f, root):
    q, carry = [0] * (len(f) - 1), 0
    for i in range(len(f) - 1, 0, -1):
        carry = (f[i] + carry * root) % R
        q[i - 1] = carry
    return q, (f[0] + carry * root) % R


def _counts(counts, n):
    counts = [counts] * (n // counts) if isinstance(counts, (int, np.integer)) else [int(c) for c in counts]
    assert sum(counts) == n and all(c >= 0 for c in counts)
    return counts


class StandInOpeningsTable(StandInFixedBase):
    """bn254.FixedBase with openings"""

    def __init__(self, oracle, bases, g2=False):
        super().__init__(oracle, bases, g2)
        self.openings_calls = []

    def openings(self, ids, counts, coeffs=None, out=None, ok_out=None):
        assert not self.closed and out is None and ok_out is None
        return on_arrays(self._openings, ids, counts, coeffs)

    def _openings(self, ids, counts, coeffs):
        ids = [v % R for v in (ids if isinstance(ids, (list, tuple)) else kints(ids))]
        counts = _counts(counts, len(ids))
        assert all(c + 1 <= self.nbase for c in counts)
        self.openings_calls.append(tuple(counts))
        pts, ok, a = np.zeros((len(ids), self.width), dtype=np.uint8), np.zeros(len(ids), dtype=np.uint8), 0
        for j, m in enumerate(counts):
            batch = ids[a:a + m]
            # the batch polynomial: the caller's row (then ok is "a root of it, and not twice"), or the product over the batch (then ok is
            # the reference's count: exactly one identity of the batch equals it)
            f = poly_from_roots(batch) if coeffs is None else [v % R for v in kints(coeffs)[j * self.nbase:j * self.nbase + m + 1]]
            for i in range(a, a + m):
                q, rem = quotient(f, ids[i])
                if coeffs is None:
                    assert (rem == 0) and (batch.count(ids[i]) >= 1)
                    if batch.count(ids[i]) != 1:
                        continue
                elif rem != 0 or sum(c * pow(ids[i], e, R) for e, c in enumerate(q)) % R == 0:
                    continue
                ok[i] = 1
                live = [c for c, v in enumerate(q) if v and self.bases[c].any()]
                if live:
                    terms = np.asarray(self.mul(self.bases[live].reshape(-1), kbytes([q[c] for c in live]), threads=4)).reshape(-1, self.width)
                    terms = terms[terms.any(1)]
                    if len(terms):
                        pts[i] = np.asarray(self.add(terms.reshape(-1))).reshape(self.width)
            a += m
        return pts, ok


class OpeningsStandIn(GTFixedStandIn):
    def FixedBase(self, bases, g2=False):
        self.tables.append(StandInOpeningsTable(self.o, bases, g2))
        return self.tables[-1]

    def fr_add(self, a, b):
        b = kints(b)
        return kbytes([x + _pick(b, i) for i, x in enumerate(kints(a))]).reshape(-1, 32)

    def fr_to_bytes(self, values):
        return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).copy()

    def fr_poly_from_roots_segments(self, roots, counts, stride, out=None):
        assert out is None
        roots = [v % R for v in (roots if isinstance(roots, (list, tuple)) else kints(roots))]
        counts, rows, a = _counts(counts, len(roots)), [], 0
        for m in counts:
            f = poly_from_roots(roots[a:a + m])
            assert len(f) <= stride
            rows += f + [0] * (stride - len(f))
            a += m
        return kbytes(rows).reshape(len(counts), stride, 32).copy()

    def fr_poly_from_roots(self, roots, B=None, out=None):
        return self.fr_poly_from_roots_segments(roots, B, B + 1)

    def fr_poly_quotients(self, coeffs, points, B, stride=None, out=None, ok=None):
        """rows of `stride` scalars, all zero with ok = 0 where the division is not exact; written into out / ok when given, as the engine's"""
        stride = B if stride is None else stride
        f, pts = np.asarray(kints(coeffs), dtype=object).reshape(-1, B + 1), kints(points)
        rows, flags = [], []
        for i, x in enumerate(pts):
            q, rem = quotient(list(f[i // B]), x % R)
            flags.append(int(rem == 0))
            rows += (q if rem == 0 else [0] * B) + [0] * (stride - B)
        q_rows, flags = kbytes(rows).reshape(len(pts), stride, 32).copy(), np.array(flags, dtype=np.uint8)
        if out is not None:
            out.reshape(-1)[:] = q_rows.reshape(-1)
            q_rows = out.reshape(len(pts), stride, 32)
        if ok is not None:
            ok[:] = flags
            flags = ok
        return q_rows, flags
