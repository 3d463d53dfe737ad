"""The GT entries' lane functions on every class of Fp12 element (tests/f12_cases.py), compiled for the host with -DGPBC_BOUNDS
(tools/bounds_check.cpp): GT.Exp in the lane-pair and the latency form, GT.Mul / Div / Inverse, the generic and the Granger-Scott
squaring, the final exponentiation in its three forms, the segmented multi-exponentiation and the fixed-base tables, each against one
big-integer statement (f12_pow with the exponent unreduced, f12_inv with 1 / 0 = 0, final_exp_direct) and against the C oracle, byte
for byte.

The functions choose their path by what the element is — Granger-Scott squarings where it is cyclotomic, the conjugate where its norm
is one — and the classes are the combinations of those answers, `norm_one_only` (norm one, NOT cyclotomic) among them: a cyclotomic
test that was really a norm-one test would square it wrongly.  Under GPBC_BOUNDS every product asserts its int64 columns and every
normalisation its limbs and a violation aborts, so a run that finishes also shows that no class leaves the limb bounds on the path it
takes.  On the host a lane pair is its own wavefront; the per-wavefront votes are the subject of tests/test_gt_classes_gpu.py."""
import numpy as np
import pytest

import bn254_py as o
from bounds_harness import hc  # noqa: F401  (the fixture)
import f12_cases as fc

GT = fc.GT
ONE = fc.to_row(o.F12_ONE)


def mismatches(got, want, idx):
    c = fc.corpus()
    return [c.describe(int(idx[j])) + " at %d" % j for j in np.nonzero((got.reshape(-1, GT) != want).any(1))[0]]


def run(fn, n, *args):
    out = np.full(n * GT + 32, 0xA5, dtype=np.uint8)
    fn(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in args[:-1]], n, out.ctypes.data, *args[-1])
    assert (out[n * GT:] == 0xA5).all()
    return out[:n * GT].reshape(n, GT)


def test_the_predicate_of_each_form_is_the_cyclotomic_equation(hc):
    """f12p_is_cyclotomic on the even and on the odd lane and wide_is_cyclotomic: the big-integer answer for every element, so `yes` for
    cyclotomic_not_gt (no order-r test), `no` for norm_one_only, -1, -e(P, Q) and every subfield element, whose difference vanishes on
    one lane's half only (in_fp6: the odd lane's C1 half), and `yes` for zero (0 * 0 == 0)"""
    c = fc.corpus()
    got = np.full((len(c), 3), 7, dtype=np.uint8)
    hc.hc_gt_is_cyclotomic(c.rows.ctypes.data, len(c), got.ctypes.data)
    bad = [c.describe(i) for i in range(len(c)) if got[i].tolist() != [c.cyclotomic[i]] * 3]
    assert not bad, bad


@pytest.mark.parametrize("entry", ["hc_gt_exp_pair", "hc_gt_exp_wide"])
def test_gt_exp_of_every_class(hc, oracle, entry):
    idx, ks = fc.class_exponent_cases()
    want = fc.want_exp(idx, ks)
    x, k = np.ascontiguousarray(fc.corpus().rows[idx]), fc.exponent_rows(ks)
    got = run(getattr(hc, entry), len(idx), x, k, ())
    assert not mismatches(got, want, idx)
    if entry == "hc_gt_exp_pair":                                       # the C oracle against the same statement, once
        assert not mismatches(oracle.gt_exp(x, k.reshape(-1), threads=8), want, idx)
        zero, r = fc.corpus().of("zero")[0], fc.EXPONENTS.index(fc.R)
        assert want[list(idx).index(zero)].tobytes() == ONE.tobytes() and not want[list(idx).index(zero) + 1:list(idx).index(zero) + 10].any()
        for cls in fc.CLASSES:                                          # x^r is one for the order-r classes alone: a reduction modulo r shows everywhere else
            at = list(idx).index(fc.corpus().of(cls)[0]) + r
            assert ks[at] == fc.R and (want[at].tobytes() == ONE.tobytes()) == (cls in fc.ORDER_R), cls


def test_mul_div_inverse_and_squarings_of_every_class(hc, oracle):
    """every element as the divisor (f12_inv_gt: the conjugate where the norm is one, the Fp6 inversion elsewhere, 1 / 0 = 0) under every
    other class as the dividend, as a factor, inverted and squared; the Granger-Scott squaring is x^2 exactly on the cyclotomic classes"""
    c = fc.corpus()
    m = len(c)
    b = np.arange(m)
    x = np.ascontiguousarray(c.rows)
    for shift in (0, 1, 7):
        a = (b + shift) % m
        xa = np.ascontiguousarray(c.rows[a])
        assert not mismatches(run(hc.hc_gt_div, m, xa, x, ()), fc.want_div(a, b), b)
        assert not mismatches(run(hc.hc_gt_mul, m, xa, x, ()), fc.want_mul(a, b), b)
    one = np.ascontiguousarray(np.tile(ONE, (m, 1)))
    assert not mismatches(run(hc.hc_gt_div, m, one, x, ()), fc.want_inverse(b), b)       # the inverse as k_gt_binary takes it
    assert not mismatches(run(hc.hc_gt_inv, m, x, ()), fc.want_inverse(b), b)
    assert not mismatches(oracle.gt_inverse(x), fc.want_inverse(b), b)
    assert not mismatches(oracle.gt_div(np.ascontiguousarray(c.rows[(b + 7) % m]), x), fc.want_div((b + 7) % m, b), b)
    assert not fc.want_inverse(c.of("zero")).any()
    squares = fc.want_exp(b, [2] * m)
    assert not mismatches(run(hc.hc_gt_sqr, m, x, (0,)), squares, b)
    gs = run(hc.hc_gt_sqr, m, x, (1,))
    wrong = (gs != squares).any(1)
    assert wrong.tolist() == [not cyc for cyc in c.cyclotomic], "Granger-Scott is x^2 on the cyclotomic classes and on nothing else in the corpus"
    assert all(wrong[i] for i in c.of("norm_one_only"))                  # why a norm-one test in place of the cyclotomic one shows


@pytest.mark.parametrize("form", ["lane", "pair", "wide"])
def test_final_exp_of_every_class(hc, oracle, form):
    """0, 1, -1, subfield elements, elements already in GT, Miller values and random ones against ONE power by s (p^12 - 1) / r: the
    conjugate-as-inverse and the Granger-Scott squarings after the easy part, and the hard part on one (no early exit)"""
    c = fc.corpus()
    b = np.arange(len(c))
    want = fc.want_final_exp(b)
    x = np.ascontiguousarray(c.rows)
    got = run(hc.hc_final_exp, len(c), x, ()) if form == "lane" else run(hc.hc_final_exp_forms, len(c), x, (int(form == "wide"),))
    assert not mismatches(got, want, b)
    if form == "lane":
        assert not mismatches(oracle.final_exp(x, threads=8), want, b)
        for i in b:
            gives_one = want[i].tobytes() == ONE.tobytes()
            if c.cls[i] in fc.EASY_PART_ONE + ("one", "minus_one"):
                assert gives_one, c.describe(i)
            if c.cls[i] in ("pairing", "pairing_inverse", "miller", "random", "cyclotomic_not_gt", "norm_one_only", "minus_pairing"):
                assert not gives_one and want[i].any(), c.describe(i)
        assert not want[c.of("zero")].any()


def test_multi_exp_groups_of_every_mix(hc):
    """groups of four that are all cyclotomic, all norm_one_only, one norm_one_only among three pairing values at each place, and every
    class four at a time, under exponents that include r and 2^256 - 1"""
    idx, ks, seg = fc.multi_exp_case(1)
    assert fc.R in ks and (1 << 256) - 1 in ks
    x, k = np.ascontiguousarray(fc.corpus().rows[idx]), fc.exponent_rows(ks)
    table = np.array(seg, dtype=np.uint64)
    n_seg = len(seg) - 1
    out = np.full(n_seg * GT + 32, 0xA5, dtype=np.uint8)
    hc.hc_gt_multi_exp_pair(x.ctypes.data, k.ctypes.data, len(ks), table.ctypes.data, len(idx), n_seg, out.ctypes.data)
    assert (out[n_seg * GT:] == 0xA5).all()
    want = fc.want_multi_exp(idx, ks, seg)
    bad = [s for s in range(n_seg) if out[s * GT:(s + 1) * GT].tobytes() != want[s].tobytes()]
    assert not bad, [(s, [fc.corpus().cls[i] for i in idx[seg[s]:seg[s + 1]]]) for s in bad]


def test_fixed_base_tables_of_every_class(hc):
    """a table per class (generic squarings whatever the base is) under r - 1, r, r + 1 and 2^256 - 1, against f12_pow"""
    c = fc.corpus()
    bases = [c.of(cls)[-1] for cls in fc.CLASSES]
    nbase, dwords = len(bases), 1 << 20
    table = np.full(nbase * dwords + 64, 0x5A5A5A5A, dtype=np.int32)
    B = np.ascontiguousarray(c.rows[bases])
    assert hc.hc_gt_fb_build(B.ctypes.data, nbase, table.ctypes.data) == 0
    assert (table[nbase * dwords:] == 0x5A5A5A5A).all()
    ks = [fc.R - 1, fc.R, fc.R + 1, (1 << 256) - 1]
    index = np.repeat(np.arange(nbase, dtype=np.uint32), len(ks))
    idx, kk = np.repeat(bases, len(ks)), ks * nbase
    n = len(idx)
    out, ok = np.full(n * GT + 32, 0xA5, dtype=np.uint8), np.full(n + 16, 0xA5, dtype=np.uint8)
    assert hc.hc_gt_fb_indexed(table.ctypes.data, nbase, index.ctypes.data, n, 1, fc.exponent_rows(kk).ctypes.data, n, out.ctypes.data, ok.ctypes.data) == 0
    assert (out[n * GT:] == 0xA5).all() and (ok[n:] == 0xA5).all() and ok[:n].all()
    assert not mismatches(out[:n * GT], fc.want_exp(idx, kk), idx)
