"""tools/check_limb_ops.hip on the device, judged here against the big integers and the limb-exact restatements of tests/limb_cases.py
(which tests/test_field_primitives.py holds against the compiled header on the CPU):
  (a) the data-dependent routines of csrc/fe29.hip.hpp on raw limbs, one case per lane: the device's rintf and float conversion, F29_KP
      in device memory, arithmetic shifts of negative limbs — over each routine's whole range of the multiplier k;
  (b) WideLds::limbs with LimbOps::norm / halve / add / sub / dbl / neg / sel at 1..7 components: the DPP wave shifts and ds_bpermute
      of the one-limb-per-lane forms, with rows that would show a carry or a parity bit crossing a component boundary;
  (c) wide_cyclo_out_limbs<true> and <false> on crafted product slots;
  (d) wide_mul / wide_sqr / wide_mul_line / wide_cyclo_sqr in the limb-parallel form against the Fe-level branch ON the device, limb for
      limb, and against big-integer Fp12 arithmetic.
The host interval harness runs the Fe-level branch only, and whole pairings meet these forms with |k| of a few units and positive
carries.  One build (into tmp when tools/check_limb_ops is missing or older than its sources), one run of the program in a child process."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bn254_py as o
import limb_cases as lc
from conftest import ROOT
from limb_cases import B, LMASK, NL, P, value

pytestmark = pytest.mark.gpu

MAGIC = 0x4C4D4231
CSRC = os.path.join(ROOT, "gopairingbasedcryptography_amd", "csrc")


def flat(rows):
    return [v for r in rows for v in r]


def fe_op_cases():
    """section A: (op, a, b, V or None, expected flag or None)"""
    red = lc.reduction_cases()
    cases = [(op, a, [0] * NL, V, None) for op in (lc.OP_REDUCE, lc.OP_REDUCE_ARITH, lc.OP_REDUCE_ARITH_NORM) for V, a in red]
    cases += [(lc.OP_CYCLO_OUT, t, x, W, None) for W, t, x in lc.cyclo_out_cases()]
    cases += [(lc.OP_CANONICAL, a, [0] * NL, V, None) for V, a in lc.canonical_cases()]
    cases += [(lc.OP_IS_ZERO, a, [0] * NL, V, want) for V, a, want in lc.is_zero_cases()]
    for op, top_bound, limb_bound in ((lc.OP_NORM, 1 << 30, lc.NORM_LIMB_BOUND), (lc.OP_MUL8_NORM, 1 << 27, lc.NORM_LIMB_BOUND), (lc.OP_HALVE, 1 << 30, lc.HALVE_LIMB_BOUND)):
        cases += [(op, a, [0] * NL, value(a), None) for a in lc.raw_cases(10 + op, top_bound, limb_bound)]
    return cases


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """cases of every section and what the device made of them"""
    tmp = tmp_path_factory.mktemp("limb_ops")
    exe, src = os.path.join(ROOT, "tools", "check_limb_ops"), os.path.join(ROOT, "tools", "check_limb_ops.hip")
    deps = [src] + [os.path.join(CSRC, f) for f in ("fe29.hip.hpp", "tower29.hip.hpp", "pairing29.hip.hpp", "wide29.hip.hpp", "wide_lds29.hip.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in deps):
        exe = str(tmp / "check_limb_ops")
        subprocess.check_call([shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + CSRC, src, "-o", exe],
                              stderr=subprocess.DEVNULL, timeout=600)
    A, Bc, C = fe_op_cases(), lc.limb_phase_cases(), lc.cyclo_out_slot_cases()
    D1, D2 = lc.wide_cases()
    words = [MAGIC, len(A), len(Bc), len(C), len(D1), len(D2)]
    for op, a, b, _, _ in A:
        words += [op] + a + b
    zero = [[0] * NL]
    for op, n_comp, a, b in Bc:
        words += [op, n_comp] + flat(a + zero * (lc.MAX_COMP - n_comp)) + flat(b + zero * (lc.MAX_COMP - n_comp))
    for alias, prod, a in C:
        words += [alias] + flat(flat(prod)) + flat(flat(a))
    for op, a, b in D1 + D2:
        words += [op] + flat(flat(a)) + flat(flat(b))
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    np.array(words, dtype="<i4").tofile(fin)
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    res = [int(v) for v in np.fromfile(fout, dtype="<i4")]
    assert len(res) == 10 * len(A) + 63 * len(Bc) + 108 * len(C) + 216 * (len(D1) + len(D2)), run.stdout
    at = [0]

    def take(n_rows):
        rows = [res[at[0] + NL * i:at[0] + NL * (i + 1)] for i in range(n_rows)]
        at[0] += NL * n_rows
        return rows
    out_a = []
    for _ in A:
        out_a.append((take(1)[0], res[at[0]]))
        at[0] += 1
    out_b = [take(7) for _ in Bc]
    out_c = [take(12) for _ in C]
    out_d = [(take(12), take(12)) for _ in D1 + D2]
    return {"A": (A, out_a), "B": (Bc, out_b), "C": (C, out_c), "D": (D1 + D2, out_d, len(D1))}


def reduced(v):
    return 100 * abs(v) < 51 * P                                      # |value| < 0.51 p, exactly


def test_a_fe_routines_on_raw_limbs(probe):
    cases, outs = probe["A"]
    for op, lo, hi in ((lc.OP_REDUCE, -255, 255), (lc.OP_REDUCE_ARITH, -255, 255), (lc.OP_REDUCE_ARITH_NORM, -255, 255), (lc.OP_CYCLO_OUT, -255, 255)):
        assert len(lc.assert_reach([V for o_, _, _, V, _ in cases if o_ == op], lo, hi)) == hi - lo + 1
    zeros = [V for o_, _, _, V, want in cases if o_ == lc.OP_IS_ZERO and want]
    assert len(lc.assert_reach(zeros, -127, 127)) == 255 and len(zeros) == 4 * 255
    assert max(abs(lc.zero_filter_remainder(a)) for o_, a, _, _, want in cases if o_ == lc.OP_IS_ZERO and want) == lc.ZERO_REMAINDER_REACHED
    assert {V // P for o_, _, _, V, _ in cases if o_ == lc.OP_CANONICAL} == set(range(-4, 4))
    assert len(cases) > 10000
    for (op, a, b, V, want), (r, flag) in zip(cases, outs):
        name = lc.OP_NAMES[op]
        if op == lc.OP_IS_ZERO:
            assert flag == int(want) == int(V % P == 0), (name, V // P, V % P, a)
            continue
        assert flag == 0
        assert r == (lc.fe_cyclo_out(a, b) if op == lc.OP_CYCLO_OUT else lc.RESTATED[op](a)), (name, a, b)
        if op in (lc.OP_REDUCE, lc.OP_REDUCE_ARITH, lc.OP_REDUCE_ARITH_NORM, lc.OP_CYCLO_OUT):
            assert (value(r) - V) % P == 0 and reduced(value(r)), (name, a, b, value(r) / P)
        elif op == lc.OP_CANONICAL:
            assert value(r) == V % P and all(0 <= v <= LMASK for v in r[:8]), (name, a)
        elif op == lc.OP_NORM:
            assert value(r) == V
        elif op == lc.OP_MUL8_NORM:
            assert value(r) == 8 * V
        else:
            assert 2 * value(r) in (V, V + P)


def test_b_one_limb_per_lane_phases(probe):
    cases, outs = probe["B"]
    assert {(op, n) for op, n, _, _ in cases} == {(op, n) for op in range(9) for n in range(1, 8)}
    # the rows the boundaries are about: a negative top limb under a zero row, all limbs -1, an odd value beside an even limb 0
    pairs = {(tuple(a[c]), tuple(a[c + 1])) for op, n, a, _ in cases if op in (lc.L_NORM, lc.L_HALVE, lc.L_HALVE_CHAIN) for c in range(n - 1)}
    assert any(lo[8] < -(1 << 28) and not any(hi) for lo, hi in pairs) and any(lo[0] & 1 and not hi[0] & 1 for lo, hi in pairs)
    assert any(lo == (-1,) * NL for lo, _ in pairs)
    for (op, n_comp, a, b), got in zip(cases, outs):
        for c in range(n_comp):
            assert got[c] == lc.limb_op(op, a[c], b[c], c), (op, n_comp, c, a, b)
        assert all(not any(row) for row in got[n_comp:])               # lanes beyond the phase wrote nothing


def test_c_cyclotomic_output_step_on_slots(probe):
    cases, outs = probe["C"]
    ks = set()
    for (alias, prod, a), got in zip(cases, outs):
        want, W = lc.cyclo_out_expected(prod, a)
        for k in range(6):
            for h in (0, 1):
                r = got[2 * k + h]
                ks.add(lc.nearest_k(W[k][h]))
                assert (value(r) - W[k][h]) % P == 0 and reduced(value(r)), (alias, k, h, value(r) / P)
                # out of fe_reduce_arith: a normalised limb (within [-2^4, 2^29 + 2^4]) minus a limb of k p in [0, 2^29) and a carry of at most 256
                assert all(-B - 512 <= v <= B + 512 for v in r[:8]) and abs(r[8]) <= lc.P8 // 2 + 270, (alias, k, h, r)
                assert r == want[k][h], (alias, k, h)
    # three times a sum of up to eleven squares, or of differences of three: far beyond what a pairing shows, on both sides
    assert ks >= set(range(-8, 9)) and min(ks) <= -50 and max(ks) >= 30, sorted(ks)


def f12_of(val):
    """six slots of two halves in tower order -> the Fp12 element of oracle/bn254_py.py (out of the 2^261 Montgomery form)"""
    s = [(lc.from_mont(sl[0]), lc.from_mont(sl[1])) for sl in val]
    return ((s[0], s[1], s[2]), (s[3], s[4], s[5]))


def cyclo_formula(x):
    """the Granger-Scott squaring FORMULA on any element: nine squares, twelve output halves"""
    a = [x[0][0], x[0][1], x[0][2], x[1][0], x[1][1], x[1][2]]
    S = [o.f2_sqr(v) for v in a] + [o.f2_sqr(o.f2_add(a[0], a[4])), o.f2_sqr(o.f2_add(a[2], a[3])), o.f2_sqr(o.f2_add(a[5], a[1]))]
    out = []
    for k in range(6):
        A, Bq = lc.CYCLO_AB[k]
        if k < 3:
            out.append(o.f2_sub(o.f2_scal(o.f2_add(o.f2_mul_xi(S[A]), S[Bq]), 3), o.f2_scal(a[k], 2)))
        else:
            d = o.f2_sub(o.f2_sub(S[lc.CYCLO_S[k]], S[A]), S[Bq])
            out.append(o.f2_add(o.f2_scal(o.f2_mul_xi(d) if k == 3 else d, 3), o.f2_scal(a[k], 2)))
    return ((out[0], out[1], out[2]), (out[3], out[4], out[5]))


def test_d_wide_operations_in_both_forms(probe):
    cases, outs, n_one = probe["D"]
    assert n_one == 64 and len(cases) == 128 and {op for op, _, _ in cases[:n_one]} == {0, 1, 2, 3} and {op for op, _, _ in cases[n_one:]} == {lc.W_MUL}
    zero = (0, 0)
    for (op, a, b), (limb_form, fe_form) in zip(cases, outs):
        assert limb_form == fe_form, op                                 # limb for limb
        x, y = f12_of(a), f12_of(b)
        if op == lc.W_MUL: want = o.f12_mul(x, y)
        elif op == lc.W_SQR: want = o.f12_sqr(x)
        elif op == lc.W_MUL_LINE: want = o.f12_mul(x, ((y[0][0], zero, zero), (y[0][1], y[0][2], zero)))
        else: want = cyclo_formula(x)
        got = f12_of([[fe_form[2 * k], fe_form[2 * k + 1]] for k in range(6)])
        assert got == want, op
        assert all(reduced(value(r)) for r in fe_form), op
