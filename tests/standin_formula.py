"""The stand-in engine of tests/standin_engine.py with the formula entries of the bn254 module added: fr_lsss_from_formula and
formula_select through the recursive restatement of tests/formula_cases.py (a code row is parsed back into its nested formula first),
and g1_sum_segments as chains of the oracle's point addition.  Nothing here shares code with formula.py or with the kernels."""
import numpy as np

import bn254_py as o
import formula_cases as fc
from standin_engine import StandInEngine


def tree_of(row):
    """the nested formula of a code row, None for a malformed one"""
    if not fc.well_formed(row):
        return None
    codes = iter(int(c) for c in row)

    def parse():
        c = next(codes)
        if c >= 0:
            return c
        left = parse()
        return ("and" if c == fc.AND else "or", left, parse())
    return parse()


class FormulaStandIn(StandInEngine):
    def fr_lsss_from_formula(self, nodes, rows, cols):
        nodes = np.asarray(nodes, dtype=np.int64)
        case = dict(trees=[tree_of(r) for r in nodes], rows=rows, cols=cols)
        matrix, rho, dims, ok = fc.expected_build(case)
        return matrix, rho, dims.astype(np.int32), ok

    def formula_select(self, nodes, held, rows):
        nodes = np.asarray(nodes, dtype=np.int64)
        nodes = nodes.reshape(-1, nodes.shape[-1])
        held = np.asarray(held, dtype=np.uint8).reshape(-1, rows)
        assert len(nodes) in (1, len(held))
        return fc.expected_select(dict(trees=[tree_of(r) for r in nodes], rows=rows, held=held, shared=len(nodes) == 1))

    def g1_sum_segments(self, pts, seg_off):
        pts, seg = np.asarray(pts, dtype=np.uint8).reshape(-1, 64), [int(v) for v in seg_off]
        out = np.zeros((len(seg) - 1, 64), dtype=np.uint8)
        for s, (a, b) in enumerate(zip(seg, seg[1:])):
            acc = None
            for p in pts[a:b]:
                acc = o.g1_add(acc, o.g1_from_bytes(p.tobytes()))
            out[s] = np.frombuffer(o.g1_to_bytes(acc), dtype=np.uint8)
        return out
