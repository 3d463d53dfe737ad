"""The stand-in engine of tests/standin_engine.py (through tests/standin_mask.py, which adds hash_to_g2 and fr_random) with the entries the
signature planners call besides: fr_dot_segments / fr_sum_segments restated once in Python integers, gt_equal as a comparison of the
rows' bytes, fr_set_bytes64 as the big-endian integer modulo r, and g1_neg from the Python oracle.  Nothing here shares code with
frdot29.hip.hpp, k_gt_equal or the planners' sequence of calls."""
import numpy as np

from sw05_fixture import kbytes, kints
from standin_engine import _neg, _rows
from standin_mask import MaskStandIn
import bn254_py as o

R = o.R


class VerifyStandIn(MaskStandIn):
    def fr_dot_segments(self, a, b, seg_off, out=None, workspace=None):
        assert out is None and workspace is None
        a, off = kints(a), [int(v) for v in np.asarray(seg_off).reshape(-1)]
        b = None if b is None else ([int(v) for v in b] if isinstance(b, (list, tuple)) else kints(b))
        assert off[0] == 0 and off[-1] == len(a) and all(x <= y for x, y in zip(off, off[1:])), "a table from 0 to n"
        shared = b is not None and len(b) != len(a)
        assert not shared or all(y - x == len(b) for x, y in zip(off, off[1:])), "a shared list needs segments of its length"
        sums = []
        for lo, hi in zip(off[:-1], off[1:]):
            sums.append(sum(a[i] * (1 if b is None else b[i - lo] if shared else b[i]) for i in range(lo, hi)))
        return kbytes(sums).reshape(-1, 32).copy()

    def fr_sum_segments(self, a, seg_off):
        return self.fr_dot_segments(a, None, seg_off)

    def gt_equal(self, a, b, out=None):
        assert out is None
        a, b = _rows(a, 384), _rows(b, 384)
        assert len(b) in (1, len(a)), "one b or one per a"
        return np.array([int(x.tobytes() == (b[i] if len(b) > 1 else b[0]).tobytes()) for i, x in enumerate(a)], dtype=np.uint8)

    def fr_set_bytes64(self, x, out=None):
        assert out is None
        rows = np.asarray(x, dtype=np.uint8).reshape(-1, 64)
        return kbytes([int.from_bytes(r.tobytes(), "big") for r in rows]).reshape(-1, 32).copy()

    def g1_neg(self, pt):
        return _neg(np.asarray(pt, dtype=np.uint8).reshape(64))
