"""The data-dependent routines of csrc/fe29.hip.hpp — fe_norm, fe_mul8_norm, fe_halve, fe_reduce, fe_reduce_arith, fe_reduce_arith_norm,
fe_cyclo_out, fe_canonical, fe_is_zero — on RAW limbs under the interval harness (tools/bounds_check.cpp: hc_fe_primitive), judged against
the big integers of tests/limb_cases.py.  The interval harness SETS the output class of a reduction (vb = 0.51, the limb intervals) and a
pairing on random points keeps the multiplier k within a few units of zero; here k runs over each routine's whole documented range, in
every signed representation its input class admits: the far rows of F29_KP, negative carries, the rounding ties of the float quotient,
+-(4p - 1) into fe_canonical, true zeros k p up to |k| = 127.  The limb-exact restatement of limb_cases, which the device test
(tests/test_limb_ops_gpu.py) judges by, is held against the compiled header here, limb for limb on every case."""
import numpy as np
import pytest

import limb_cases as lc
from limb_cases import B, LMASK, NL, P, value
from bounds_harness import hc  # noqa: F401  (the fixture)


def vb_of(V, below):
    """|V| / p as the harness's double, a hair up — but inside the routine's OPEN class |value| < below * p, which a double cannot state
    closer than its last place"""
    return min(abs(V) / P * (1 + 1e-12) + 1e-12, float(np.nextafter(below, 0)))


def run(hc, op, rows, slack, below, rows_b=None):
    a = np.ascontiguousarray(rows, dtype=np.int32)
    b = np.ascontiguousarray(rows_b if rows_b is not None else np.zeros_like(a), dtype=np.int32)
    vb = np.zeros((len(a), 2))
    vb[:, 0] = [vb_of(value(r), below) for r in rows]
    if rows_b is not None:
        vb[:, 1] = [vb_of(value(r), below) for r in rows_b]
    out, flags = np.zeros_like(a), np.zeros(len(a), dtype=np.int32)
    assert hc.hc_fe_primitive(op, a.ctypes.data, b.ctypes.data, len(a), slack, vb.ctypes.data, out.ctypes.data, flags.ctypes.data) == 0
    return [[int(v) for v in r] for r in out], [int(f) for f in flags]


def reduced(v):
    return 100 * abs(v) < 51 * P                                      # |value| < 0.51 p, exactly


def test_the_cases_reach_what_they_claim():
    assert len(lc.assert_reach([V for V, _ in lc.reduction_cases()], -255, 255)) == 511
    assert len(lc.assert_reach([V for V, _ in lc.reduction_cases(5, 255, 512, -512)], -255, 255)) == 511
    assert len(lc.assert_reach([W for W, _, _ in lc.cyclo_out_cases()], -255, 255)) == 511
    zeros = [V for V, _, z in lc.is_zero_cases() if z]
    assert all(V % P == 0 for V in zeros) and len(lc.assert_reach(zeros, -127, 127)) == 255
    assert all(V % P for V, _, z in lc.is_zero_cases() if not z)
    can = [V for V, _ in lc.canonical_cases()]
    assert {V // P for V in can} == set(range(-4, 4)) and 4 * P - 1 in can and 1 - 4 * P in can
    # rounding ties: top limbs within four units of (k + 1/2) P8, for every k of the range
    ties = {(2 * r[8]) // (2 * lc.P8) for _, r in lc.reduction_cases() if abs((2 * r[8]) % (2 * lc.P8) - lc.P8) <= 8}
    assert ties >= set(range(-255, 255))
    # negative carries and every mode: limbs below zero, limbs above 2^29, and limbs at both ends of the class
    limbs = [v for _, r in lc.reduction_cases() for v in r[:8]]
    assert min(limbs) == -B - 1024 and max(limbs) == B + 1024 and sum(v < 0 for v in limbs) > len(limbs) // 8


@pytest.mark.parametrize("op", [lc.OP_REDUCE, lc.OP_REDUCE_ARITH, lc.OP_REDUCE_ARITH_NORM])
def test_reductions_over_the_whole_range_of_k(hc, op):
    # (cases, slack, lowest input limb): every signed representation of slack 1024, and the weakly normalised class [-2^9, 2^29 + 2^9]
    for cases, slack, floor in ((lc.reduction_cases(), 1024, -B - 1024), (lc.reduction_cases(5, 255, 512, -512), 512, -512)):
        out, _ = run(hc, op, [r for _, r in cases], slack, 256.0)
        for (V, a), r in zip(cases, out):
            assert value(a) == V
            assert r == lc.RESTATED[op](a), (lc.OP_NAMES[op], a)
            assert (value(r) - V) % P == 0 and reduced(value(r)), (lc.OP_NAMES[op], a, value(r) / P)
            assert abs(r[8]) <= lc.P8 // 2 + 270
            if op == lc.OP_REDUCE_ARITH_NORM:
                # out of fe_norm: limb 0 masked; limb i >= 1 a masked limb plus the carry of a_(i-1) - (limb of k p) - (its carry, |.| <= 256)
                lo_c, hi_c = (floor - LMASK - 256) >> lc.LB, (B + slack + 256) >> lc.LB
                assert (lo_c, hi_c) == ((-3, 1) if slack == 1024 else (-2, 1))
                assert 0 <= r[0] <= LMASK and all(lo_c <= v <= LMASK + hi_c for v in r[1:8]), r
            else:
                # an input limb minus a limb of k p in [0, 2^29) (and, in the arithmetic form, a carry of at most 256 either way)
                assert all(floor - LMASK - 256 <= v <= B + slack + 256 for v in r[:8]), r
                if op == lc.OP_REDUCE and slack == 512:
                    assert all(abs(v) <= B + 512 for v in r[:8]), r   # the class the header states, for the inputs it states it for


def test_cyclo_out(hc):
    cases = lc.cyclo_out_cases()
    out, _ = run(hc, lc.OP_CYCLO_OUT, [t for _, t, _ in cases], 16, 256.0 / 3, [x for _, _, x in cases])
    for (W, t, x), r in zip(cases, out):
        assert 3 * value(t) - 2 * value(x) == W and min(t[:8] + x[:8]) >= -16 and max(t[:8] + x[:8]) <= B + 16
        assert r == lc.fe_cyclo_out(t, x), (t, x)
        assert (value(r) - W) % P == 0 and reduced(value(r)), (t, x, value(r) / P)
        # fe_norm of 3 t - 2 x - row: carries of limbs within [-3 * 2^29 - 80, 3 * 2^29 + 80]
        assert 0 <= r[0] <= LMASK and all(-4 <= v <= LMASK + 3 for v in r[1:8]) and abs(r[8]) <= lc.P8 // 2 + 270, r


def test_canonical(hc):
    cases = lc.canonical_cases()
    out, _ = run(hc, lc.OP_CANONICAL, [r for _, r in cases], 1024, 4.0)
    for (V, a), r in zip(cases, out):
        assert value(a) == V and r == lc.fe_canonical(a), (V, a)
        assert value(r) == V % P and all(0 <= v <= LMASK for v in r[:8]) and 0 <= r[8] <= lc.P8, (V, r)


def test_is_zero(hc):
    cases = lc.is_zero_cases()
    _, flags = run(hc, lc.OP_IS_ZERO, [r for _, r, _ in cases], 64, 128.0)
    for (V, a, want), got in zip(cases, flags):
        assert value(a) == V and bool(got) == want == (V % P == 0), (V // P, V % P, a)
    assert sum(want for _, _, want in cases) == 4 * 255
    # how far into the filter's window (136) the true zeros reach: 57 of the 59 the class allows
    assert lc.ZERO_REMAINDER_REACHED == 57 and max(abs(lc.zero_filter_remainder(a)) for _, a, want in cases if want) == 57


def test_norm_mul8_halve(hc):
    for op, top_bound, limb_bound in ((lc.OP_NORM, 1 << 30, lc.NORM_LIMB_BOUND), (lc.OP_MUL8_NORM, 1 << 27, lc.NORM_LIMB_BOUND), (lc.OP_HALVE, 1 << 30, lc.HALVE_LIMB_BOUND)):
        rows = lc.raw_cases(10 + op, top_bound, limb_bound)
        assert [-1] * NL in rows and any(r[i] == 0 and r[i + 1] < 0 for r in rows for i in range(7))
        out, _ = run(hc, op, rows, limb_bound - B, 1e6)
        for a, r in zip(rows, out):
            assert r == lc.RESTATED[op](a), (lc.OP_NAMES[op], a)
            if op == lc.OP_NORM:
                assert value(r) == value(a) and 0 <= r[0] <= LMASK and all(-3 <= v <= LMASK + 2 for v in r[1:8]), a
            elif op == lc.OP_MUL8_NORM:
                assert value(r) == 8 * value(a) and 0 <= r[0] <= LMASK - 7 and all(-24 <= v <= LMASK - 7 + 23 for v in r[1:8]), a
            else:
                assert 2 * value(r) in (value(a), value(a) + P) and (2 * value(r) - value(a)) % P == 0, a
