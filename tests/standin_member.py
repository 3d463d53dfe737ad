"""The stand-in engine of tests/standin_verify.py with the entries agka09.py calls besides: hash_to_g1 from the Python oracle, the segment
sums g1_sum_segments / g2_sum_segments as the oracle's sum per segment, gt_prod as a chain of the oracle's gt_mul per segment, and the
membership verdicts as tests/member_cases.py states them in Python integers (a stored value not below p: 0; the curve equations; [r]Q by
plain double-and-add; z != 0 and z^r == 1).  Nothing here shares code with member29.hip.hpp or with the planner's sequence of calls."""
import numpy as np

import bn254_py as o
import member_cases as mc
from standin_engine import GT_ONE, _rows
from standin_verify import VerifyStandIn


def _segments(seg_off):
    off = [int(v) for v in np.asarray(seg_off).reshape(-1)]
    return list(zip(off[:-1], off[1:]))


class MemberStandIn(VerifyStandIn):
    def hash_to_g1(self, msgs, dst, msg_off=None):
        if msg_off is not None:
            buf = np.asarray(msgs, dtype=np.uint8).tobytes()
            msgs = [buf[int(a):int(b)] for a, b in zip(msg_off[:-1], msg_off[1:])]
        pts = [np.frombuffer(o.g1_to_bytes(o.hash_to_g1(bytes(m), bytes(dst))), dtype=np.uint8) for m in msgs]
        return np.stack(pts) if pts else np.zeros((0, 64), dtype=np.uint8)

    def _sum_segments(self, pts, seg_off, width):
        pts, add = _rows(pts, width), self.o.g1_sum if width == 64 else self.o.g2_sum
        out = np.zeros((len(_segments(seg_off)), width), dtype=np.uint8)
        for s, (a, b) in enumerate(_segments(seg_off)):
            if b > a:
                out[s] = np.asarray(add(pts[a:b].reshape(-1))).reshape(width)
        return out

    def g1_sum_segments(self, pts, seg_off): return self._sum_segments(pts, seg_off, 64)
    def g2_sum_segments(self, pts, seg_off): return self._sum_segments(pts, seg_off, 128)

    def gt_prod(self, x, seg_off=None):
        x = _rows(x, 384)
        out = []
        for a, b in _segments([0, len(x)] if seg_off is None else seg_off):
            acc = GT_ONE
            for i in range(a, b):
                acc = np.asarray(self.o.gt_mul(acc, x[i])).reshape(384)
            out.append(acc)
        return out[0] if seg_off is None else np.stack(out)

    # ---- membership, in Python integers
    def g1_is_on_curve(self, x, out=None):
        assert out is None
        return np.array([int(mc.canonical(b) and o.g1_is_on_curve(o.g1_from_bytes(b))) for b in (r.tobytes() for r in _rows(x, 64))], dtype=np.uint8)

    g1_is_in_subgroup = g1_is_on_curve

    def g2_is_on_curve(self, x, out=None):
        assert out is None
        return np.array([int(mc.canonical(b) and o.g2_is_on_curve(o.g2_from_bytes(b))) for b in (r.tobytes() for r in _rows(x, 128))], dtype=np.uint8)

    def g2_is_in_subgroup(self, x, out=None):
        assert out is None
        return np.array([int(mc.canonical(b) and o.g2_in_subgroup(o.g2_from_bytes(b))) for b in (r.tobytes() for r in _rows(x, 128))], dtype=np.uint8)

    def gt_is_in_subgroup(self, x, out=None):
        assert out is None
        return np.array([mc.gt_truth(r.tobytes()) for r in _rows(x, 384)], dtype=np.uint8)
