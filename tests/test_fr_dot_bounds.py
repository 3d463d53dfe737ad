"""The accumulation bound of the segmented inner products in Fr on the CPU: csrc/frdot29.hip.hpp compiled for the host with -DGPBC_BOUNDS
(tools/bounds_check.cpp: hc_fr_dot_segments runs the plan of csrc/segred29.hip.hpp, fr_dot_lane for the 64 lanes of every wavefront with
8 to 64 lanes per piece, the fold steps and fr_dot_store) against Python integers, exactly.  Under GPBC_BOUNDS every product asserts its int64 columns, every
normalisation its limbs and fr_canonical its input range, for the interval classes of the operands and not for the values of a run, and
a violation aborts: a run that finishes is the overflow proof.  A lane's intervals grow with the rounds it takes between two reductions
and are reset by a reduction, so the proof needs a piece that passes FR_DOT_RUN_MUL (FR_DOT_RUN_SUM) rounds; the cases hold one, and the
values at their largest (2^256 - 1 everywhere) show that the arithmetic agrees with the intervals there."""
import ctypes

import numpy as np
import pytest

from bounds_harness import hc  # noqa: F401  (the fixture)
import fr_dot_cases as fc

GUARD = 0xA5


def run(hc, a, b, seg, n=None):
    a = np.ascontiguousarray(a).reshape(-1)
    n = a.size // 32 if n is None else n
    n_seg = len(seg) - 1
    seg = np.ascontiguousarray(seg, dtype=np.uint64)
    out = np.full(32 * n_seg + 16, GUARD, dtype=np.uint8)
    lv = (ctypes.c_uint32 * 2)()
    bb = None if b is None else np.ascontiguousarray(b).reshape(-1)
    rc = hc.hc_fr_dot_segments(a.ctypes.data, None if bb is None else bb.ctypes.data, 0 if bb is None else bb.size // 32, seg.ctypes.data, n, n_seg,
                               out.ctypes.data, ctypes.addressof(lv))
    assert rc == 0 and (out[32 * n_seg:] == GUARD).all()
    return out[:32 * n_seg].reshape(n_seg, 32), lv[0], lv[1]


def test_the_case_file_restates_the_headers_constants(hc):
    o = (ctypes.c_uint32 * 8)()
    hc.hc_fr_dot_shape(o)
    assert list(o) == [fc.FILL, fc.GROUP, fc.PLAIN_MIN, fc.WAVE, fc.NORM, fc.RUN_MUL, fc.RUN_SUM, fc.LANES_MIN]


@pytest.mark.parametrize("name", [c for c in fc.CASES if c != "three_levels"])
def test_cases_equal_python_integers(hc, name):
    lengths = fc.CASES[name][0]
    for mode in fc.case_modes(lengths):
        a, b, seg, shared = fc.case_inputs(name, mode)
        got, lv, used = run(hc, a, b, seg)
        assert lv == len(fc.levels(len(a), len(lengths), b is not None)), (name, mode)
        want_lanes = 0
        for L in fc.launch_lanes(len(a), len(lengths), b is not None):
            want_lanes |= L
        assert used == want_lanes, (name, mode)
        assert got.tobytes() == fc.expect(a, b, seg, shared=shared).tobytes(), (name, mode)


@pytest.mark.parametrize("value", sorted(fc.EXTREMES))
def test_the_longest_run_with_every_operand_at_its_largest(hc, value):
    """62 rounds in one piece: a lane takes FR_DOT_RUN_MUL rounds of two products (FR_DOT_RUN_SUM rounds of two summands) between two
    reductions, then the closing product, the fold of 64 such lanes and the canonical form — with 2^256 - 1 in every operand the values
    sit at the top of the classes the intervals are stated for"""
    a, b, seg = fc.extreme_inputs(fc.EXTREMES[value])
    assert fc.rounds(int(seg[1])) > fc.RUN_MUL > fc.RUN_SUM
    for bb in (b, None):
        got, lv, used = run(hc, a, bb, seg)
        assert lv == 1 and used == fc.WAVE and got.tobytes() == fc.expect(a, bb, seg).tobytes()
        assert all(v < fc.R for v in fc.ints(got))


def test_the_stated_bounds_follow_from_the_limb_bounds():
    """the arithmetic of the header's comment, from the limb bounds of a product and the normalisation interval"""
    limb = 1 << 29
    eps = 2 * (2**256 / fc.R) ** 2 * fc.R / 2**261                       # a round of two products of raw operands
    assert 2**256 / fc.R < 5.3 and eps < 0.34
    # limbs: a normalised accumulator (below 2^29 + 4) plus FR_DOT_NORM rounds of limbs below 2^29 stays in int32
    assert limb + 4 + fc.NORM * limb < 2**31
    # ... and without a second operand: a round is the sum of two raw operands, normalised after every round
    assert limb + 4 + 2 * limb < 2**31
    # value: FR_DOT_RUN_MUL rounds on top of a reduced value, top limb (bits 232 and up) below 2^28
    reduced = 1 + 45 * fc.R / 2**261
    top_mul, top_sum = reduced + fc.RUN_MUL * (1 + eps), reduced + fc.RUN_SUM * 2 * 5.3
    assert reduced < 1.27 and top_mul < 45 and top_sum < 45
    assert 45 * fc.R / 2**232 < 2**28
    # the closing product and the reduction: nine columns of a normalised limb by a limb of a constant
    assert 9 * (limb + 4) * limb < 2**62
    # the fold: 64 lane results in (-0.27 r, 1.27 r); the last reduction leaves eps < 0.49 and fr_canonical<1, 2> takes [-r, 2 r)
    assert fc.WAVE * 1.27 < 82 and 82 * fc.R / 2**261 < 0.49 and 82 * fc.R / 2**232 < 2**28
