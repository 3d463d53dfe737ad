"""The seven-product sparse line multiplication of the lane-pair Miller accumulator (four products at c0 = 1) against the
eight-product (five-product) form it replaces, on the same operands, in the -DGPBC_BOUNDS host build of the device headers
(tools/bounds_check.cpp hc_sparse_products).  In that build every product asserts that its int64 columns cannot overflow for ANY
value inside the operands' limb intervals, so a run that finishes is the overflow proof for the operand class; the values are
compared bit for bit after the form's correction: f12p_mul_034_x2 returns twice the product (the Miller loop folds the twos into
the constant of its last line), f12p_mul_34_half takes half the line and returns the product itself.  CPU only."""
import ctypes
import json
import os

import numpy as np
import pytest

import bn254_py as o
from conftest import ROOT
from bounds_harness import hc  # noqa: F401  (the fixture)

NL, LB = 9, 29
LMASK = (1 << LB) - 1
P8 = o.P >> (LB * (NL - 1))                    # top limb of p
RP = 1 << (LB * NL)                            # internal Montgomery radix 2^261
TOP = P8 // 2 - 2                              # |top limb| of a value-reduced element (|value| < 0.51 p)
# executed v_mad_i64_i32 of one Miller loop (line phase + both accumulator lanes) BEFORE the seven-product form:
# profiles/executed_mads.json "miller_loop" of the parent commit
PARENT_MILLER_MADS = 1482678
F2_PRODUCT_MADS = 486                          # one F2 leaf: 4 x 81 limb products + 2 x 81 reduction terms
MILLER_LINES = 88


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def accumulators():
    """Raw limbs [case][lane][6 Fp][9] of positive-normalised accumulators (limb 0 in [0, 2^29), limbs 1..7 in [-2^4, 2^29 + 2^4],
    the sign in the top limb, |value| < 0.51 p): 256 random ones and the extremes of the class."""
    rng = np.random.default_rng(7)
    rnd = rng.integers(0, 1 << LB, size=(256, 2, 6, NL), dtype=np.int64)
    rnd[..., NL - 1] = rng.integers(-TOP, TOP + 1, size=(256, 2, 6))

    def const(low0, low, top):
        h = np.full((2, 6, NL), low, dtype=np.int64)
        h[..., 0], h[..., NL - 1] = low0, top
        return h
    ext = [const(LMASK, LMASK + 16, TOP),        # every limb at the top of the class
           const(0, -16, -TOP),                  # every limb at the bottom
           const(LMASK, LMASK + 16, -TOP),       # negative values carried in the top limb, low limbs as large as they get
           const(0, 0, -1),                      # -2^232
           const(0, -16, TOP)]
    mixed = rnd[0].copy()                        # random low limbs under a negative top limb
    mixed[..., NL - 1] = -TOP
    ext.append(mixed)
    return rnd, np.stack(ext)


def fp_bytes(v):
    return (v * o.MONT_R % o.P).to_bytes(32, "little")


def lines(n_random, rng):
    """(c0, c3, u, w) with c4 = u - w, as gnark E2 bytes; returns the byte rows and the values (c0, c3, c4)."""
    rf2 = lambda: (int.from_bytes(rng.bytes(32), "little") % o.P, int.from_bytes(rng.bytes(32), "little") % o.P)
    z = (0, 0)
    rows = []
    for _ in range(n_random):
        rows.append((rf2(), rf2(), rf2(), rf2()))
    c3, u = rf2(), rf2()
    rows += [(rf2(), c3, c3, z),                 # c3 = c4
             (rf2(), c3, z, c3),                 # c3 = -c4
             (rf2(), c3, z, z),                  # c4 = 0
             (rf2(), c3, u, u),                  # c4 = 0 as a difference of two equal values
             (z, c3, rf2(), rf2())]              # c0 = 0
    return rows


def pack_lines(rows):
    return np.frombuffer(b"".join(fp_bytes(c) for r in rows for f in r for c in f), dtype=np.uint8).copy()


def fp_out(buf):
    return [int.from_bytes(buf[32 * i:32 * i + 32].tobytes(), "little") for i in range(len(buf) // 32)]


def acc_value(h):
    """[lane][6][9] raw limbs -> the Fp12 value ((b0, b1, b2), (b0, b1, b2)) in plain integers"""
    rinv = pow(RP, -1, o.P)
    fe = lambda w: sum(int(x) << (LB * i) for i, x in enumerate(w)) * rinv % o.P
    return tuple(tuple((fe(h[lane][2 * k]), fe(h[lane][2 * k + 1])) for k in range(3)) for lane in range(2))


@pytest.fixture(scope="module")
def cases():
    rnd, ext = accumulators()
    rng = np.random.default_rng(11)
    special = lines(0, rng)
    # every extreme accumulator with every special line and two random ones; the random accumulators with a random line each and
    # the special lines in turn
    H, L = [], []
    for h in ext:
        for l in special + lines(2, rng)[:2]:
            H.append(h); L.append(l)
    rl = lines(len(rnd), rng)[:len(rnd)]
    for i, h in enumerate(rnd):
        H.append(h); L.append(special[i % len(special)] if i % 4 == 3 else rl[i])
    return np.stack(H).astype(np.int32), L


@pytest.mark.parametrize("one", [0, 1], ids=["f12p_mul_034_x2", "f12p_mul_34_half"])
def test_new_sparse_product_equals_old(hc, cases, one):
    H, L = cases
    n = len(L)
    Lb = pack_lines(L)
    old, new = np.zeros(n * 384, dtype=np.uint8), np.zeros(n * 384, dtype=np.uint8)
    hc.hc_sparse_products(vp(H), vp(Lb), ctypes.c_size_t(n), ctypes.c_int(one), vp(old), vp(new))   # aborts on a bounds violation
    a, b = fp_out(old), fp_out(new)
    assert any(a)
    if one:
        assert a == b
    else:
        assert [2 * x % o.P for x in a] == b
    # ... and the old form is the product it claims to be (a few of each kind against the Python tower)
    for i in list(range(0, 42, 5)) + [n - 1, n - 2]:
        c0, c3, u, w = L[i]
        c4 = ((u[0] - w[0]) % o.P, (u[1] - w[1]) % o.P)
        line = (((1, 0) if one else c0, (0, 0), (0, 0)), (c3, c4, (0, 0)))
        assert old[384 * i:384 * (i + 1)].tobytes() == o.gt_to_bytes(o.f12_mul(acc_value(H[i]), line)), i


def test_miller_loop_mad_count_drops_by_one_leaf_per_sparse_product(hc):
    """Every sparse product of the accumulator loses exactly one F2 leaf (486 MADs) on each of the two lanes and nothing else
    changes: the line phase multiplies by other constants, not more often.  A Miller loop has 88 lines; the first one seeds the
    accumulator and the other 87 are multiplied in, so the count falls by 87 x 486 x 2 = 84 564 from the parent's 1 482 678.
    (The issue states 88 x 486 x 2: it counted the lines, not the products.)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import executed_mads
    got = executed_mads.count(hc, n=4)["miller_loop"]
    naf = [int(x) for x in __import__("re").search(r"#define BN254_ATE_NAF \{([^}]*)\}", open(os.path.join(
        ROOT, "gopairingbasedcryptography_amd", "csrc", "bn254_constants.hip.hpp")).read()).group(1).split(",")]
    n_lines = (len(naf) - 1) + sum(1 for d in naf[:-1] if d) + 2
    assert n_lines == MILLER_LINES
    assert got == PARENT_MILLER_MADS - (n_lines - 1) * F2_PRODUCT_MADS * 2
    doc = json.load(open(os.path.join(ROOT, "profiles", "executed_mads.json")))
    assert doc["mads_per_unit"]["miller_loop"] == got
