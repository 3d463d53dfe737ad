"""The stand-in engine of tests/standin_engine.py with the entries bf01.py calls besides: hash_to_g2 from the Python oracle
(oracle/bn254_py.py), gt_xor_mask as tests/mask_cases.py states it — the oracle's GT.Bytes() XOR the message, cut to the shorter, zero
beyond, an item at a time — in the three message forms of bn254.gt_xor_mask, and fr_random from the oracle of tests/chacha_cases.py with
every draw written down.  multi_pair_fixed_q is StandInEngine's.  Nothing here shares code with mask29.hip.hpp or with the planner's
sequence of calls."""
import numpy as np

import bn254_py as o
import chacha_cases as cc
import mask_cases as mc
from standin_engine import StandInEngine, _rows


class MaskStandIn(StandInEngine):
    def __init__(self, oracle, without=()):
        super().__init__(oracle, without)
        self.draws = []

    def hash_to_g2(self, msgs, dst, msg_off=None):
        if msg_off is not None:
            buf = np.asarray(msgs, dtype=np.uint8).tobytes()
            msgs = [buf[int(a):int(b)] for a, b in zip(msg_off[:-1], msg_off[1:])]
        pts = [np.frombuffer(o.g2_to_bytes(o.hash_to_g2(bytes(m), bytes(dst))), dtype=np.uint8) for m in msgs]
        return np.stack(pts) if pts else np.zeros((0, 128), dtype=np.uint8)

    def gt_xor_mask(self, gt, msgs, msg_off=None, out=None):
        assert out is None
        gt = _rows(gt, 384)
        if msg_off is None and isinstance(msgs, (list, tuple)):
            items, form = [bytes(m) for m in msgs], "list"
        elif msg_off is None:
            assert isinstance(msgs, np.ndarray) and msgs.ndim == 2, "messages without offsets are a list or rows"
            items, form = [r.tobytes() for r in msgs], "rows"
        else:
            buf, off = np.asarray(msgs, dtype=np.uint8).reshape(-1), [int(v) for v in np.asarray(msg_off).reshape(-1)]
            items, form = [buf[a:b].tobytes() for a, b in zip(off[:-1], off[1:])], "flat"
        assert len(items) == len(gt), "one GT element per message"
        res = [mc.xor_cut(m, mc.mask_of(g)) for m, g in zip(items, gt)]
        lens = np.array([L for _, L in res], dtype=np.uint32)
        if form == "rows":
            return np.frombuffer(b"".join(x for x, _ in res), dtype=np.uint8).reshape(msgs.shape).copy(), lens
        if form == "list":
            offs = np.zeros(len(items) + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(m) for m in items], dtype=np.uint64)
            return (np.frombuffer(b"".join(x for x, _ in res), dtype=np.uint8).copy(), offs), lens
        flat = np.array(buf, copy=True)
        for (x, _), a in zip(res, off[:-1]):
            flat[a:a + len(x)] = np.frombuffer(x, dtype=np.uint8)
        return flat, lens

    def fr_random(self, seed, n, stream=0, first=0, out=None, like=None):
        self.draws.append((n, stream, first))
        return cc.scalars(bytes(seed), stream, first, n)
