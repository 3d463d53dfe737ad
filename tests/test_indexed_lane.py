"""The lane functions of the indexed fixed-base sums (csrc/fbindex29.hip.hpp) and of LSSS share generation (csrc/lsss29.hip.hpp) as the
kernels launch them — geometry, staging into a checked stand-in for the LDS block, lane-to-output mapping, workgroup by workgroup —
compiled for the host with -DGPBC_BOUNDS (tools/bounds_check.cpp: hc_fb_indexed, hc_fr_lsss_shares), on the cases of
tests/indexed_cases.py: shares against Python integers, points against the oracle's scalar multiplication and sum over the selected
bases, exactly.  Every product in that build asserts its int64 columns for ANY input of its interval class and every canonical form
its input range, so a run that finishes is the overflow proof of the accumulator's bound (the header comment of lsss29.hip.hpp)."""
import ctypes

import numpy as np
import pytest

from bounds_harness import hc  # noqa: F401  (the fixture)
import indexed_cases as ic

VP = ctypes.c_void_p
R = ic.R


def run_shares(hc, case, geoms=None):
    m, v = ic.matrix_rows(case), ic.vector_rows(case)
    k, rows = case["k"], case["rows"]
    out = np.full((k * rows + 1, 32), 0xA5, dtype=np.uint8)
    geom = np.zeros(6, dtype=np.uint32)
    assert hc.hc_fr_lsss_shares(m.ctypes.data, case["nm"], rows, case["cols"], v.ctypes.data, k, out.ctypes.data, geom.ctypes.data) == 0
    assert (out[k * rows] == 0xA5).all() and geom[5] == k * rows                  # every output's lane ran exactly once, nothing past the end
    if geoms is not None:
        geoms.append(tuple(int(x) for x in geom[:5]))
    return ic.ints(out[:k * rows])


@pytest.mark.parametrize("rows,cols", ic.SHARE_SHAPES)
@pytest.mark.parametrize("per_item", [False, True], ids=["shared", "per-item"])
def test_shares_as_launched(hc, rows, cols, per_item):
    for k in (1, 3, 67):
        case = ic.shares_case(rows, cols, k, per_item)
        assert run_shares(hc, case) == [v for r in case["want"] for v in r], (rows, cols, k)


def test_share_values_act_as_residues(hc):
    """r and 2^256 - 1 are 0 and 2^256 - 1 - 5 r; -1 arrives as r - 1; an all-zero matrix gives zero shares"""
    top = ic.TOP % R
    case = {"matrix": [[[R, ic.TOP, R - 1], [0, 0, 0]]], "vectors": [[5, ic.TOP, R - 1], [R + 1, 1, 1]], "rows": 2, "cols": 3, "k": 2, "nm": 1}
    assert run_shares(hc, case) == [(top * top + 1) % R, 0, (top - 1) % R, 0]


def test_share_geometry(hc):
    """(rows per group, row groups, items per workgroup, pitch, workgroups) of the shapes that take each path"""
    geoms = []
    for rows, cols, k, per_item in ((1, 1, 67, False), (4, 3, 67, False), (16, 15, 67, False), (64, 64, 3, False), (64, 64, 3, True), (33, 9, 5, False), (16, 15, 1, False), (5, 64, 9, False)):
        run_shares(hc, ic.shares_case(rows, cols, k, per_item), geoms)
    assert geoms == [(1, 1, 64, 9, 2), (4, 1, 16, 27, 5), (16, 1, 4, 135, 17), (4, 16, 16, 577, 16), (64, 1, 1, 577, 3), (28, 2, 2, 81, 6), (16, 1, 4, 135, 1), (4, 2, 16, 577, 2)]


def test_share_bound_margins(hc):
    """the largest sum the entry allows, 64 columns of (2^256 - 1)^2: columns, limbs and value stay inside what the header states"""
    st = np.zeros(7)
    case = {"matrix": [[[ic.TOP] * 64] * 64], "vectors": [[ic.TOP] * 64] * 2, "rows": 64, "cols": 64, "k": 2, "nm": 1}
    assert run_shares(hc, case) == [64 * (ic.TOP % R) ** 2 % R] * 128
    hc.hc_stats(st.ctypes.data_as(VP))
    assert 0 < st[0] < 2.0**63 and st[1] < 2.0**31


def test_share_harness_refuses_malformed_arguments(hc):
    z = np.zeros(64 * 32, dtype=np.uint8)
    p = z.ctypes.data
    for args in ((p, 1, 0, 1, p, 1), (p, 1, 65, 1, p, 1), (p, 1, 1, 0, p, 1), (p, 1, 1, 65, p, 1), (p, 2, 1, 1, p, 3), (p, 1, 1, 1, p, 0), (None, 1, 1, 1, p, 1)):
        assert hc.hc_fr_lsss_shares(*args, p, None) == -1, args


# ------------------------------------------------------------------------------------------------ indexed sums
def run_indexed(hc, oracle, g2, case, group_min=0, ok_out=True):
    b = ic.bases(oracle, g2)
    width, n = 128 if g2 else 64, case["n"]
    k = ic.rows([v for r in case["scalars"] for v in r])
    out = np.full((n + 1, width), 0xA5, dtype=np.uint8)
    ok = np.full(n + 1, 7, dtype=np.uint8)
    geom = np.zeros(3, dtype=np.uint32)
    idx = np.ascontiguousarray(case["index"])
    rc = hc.hc_fb_indexed(int(g2), b.ctypes.data, ic.NBASE, idx.ctypes.data, case["P"], case["terms"], k.ctypes.data, n, group_min, out.ctypes.data,
                          ok.ctypes.data if ok_out else None, geom.ctypes.data)
    assert rc == 0 and (out[n] == 0xA5).all() and ok[n] == 7 and geom[2] == n
    return out[:n], ok[:n], tuple(int(v) for v in geom)


# (G2, terms, outputs, index rows): the host build of a G2 table row under the interval harness takes milliseconds, so G2 gets the two
# shapes that reach every branch and G1 the spread
CASES = [(False, 1, 23, 23), (False, 2, 23, 23), (False, 3, 23, 23), (False, 2, 40, 19), (False, 2, 9, 1), (False, 16, 3, 3), (False, 1, 40, 19),
         (True, 2, 19, 19), (True, 1, 17, 16)]


@pytest.mark.parametrize("g2,terms,n,P", CASES)
def test_indexed_lane_against_the_oracle(hc, oracle, g2, terms, n, P):
    case = ic.indexed_case(n, terms, P)
    want, want_ok = ic.expected(oracle, g2, case)
    got, ok, _ = run_indexed(hc, oracle, g2, case)
    assert ok.tolist() == want_ok.tolist()
    bad = [i for i in range(n) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, (bad, case["planted"])
    if P >= 16:
        assert (want_ok == 0).sum() >= 2 and not got[want_ok == 0].any()              # the two invalid index rows: all-zero outputs


def test_indexed_corpus_covers_what_it_claims():
    for terms in (2, 3, 16):
        c = ic.indexed_case(323, terms, 323)
        assert {"special", "ends", "cancel", "double", "double-one", "equal-bases", "all-none", "inf-base", "index-nbase", "index-fffffffe"} <= set(c["planted"])
    c = ic.indexed_case(323, 1, 19)
    assert {"special", "ends", "all-none", "index-nbase", "index-fffffffe"} <= set(c["planted"])
    assert "index-nbase" not in ic.indexed_case(323, 2, 1)["planted"]                     # one shared row stays valid
    assert (ic.indexed_case(323, 2, 19)["index"] == ic.NONE).any()


def test_both_lane_orders_give_the_same_outputs(hc, oracle):
    """periodic rows: the grouped order (a workgroup's lanes share the index row) and the natural order own every output exactly once
    and compute the same bytes; without ok_out the outputs are the same"""
    case = ic.indexed_case(200, 2, 3, invalid=False)
    case["scalars"] = [[v & 0xFFFF for v in r] for r in case["scalars"]]                 # two windows: the table rows to build stay few
    a, ok_a, ga = run_indexed(hc, oracle, False, case, group_min=64)
    b, ok_b, gb = run_indexed(hc, oracle, False, case, group_min=1 << 40)
    c, _, _ = run_indexed(hc, oracle, False, case, group_min=64, ok_out=False)
    assert ga == (1, 6, 200) and gb == (0, 4, 200)                                        # 3 rows x 2 workgroups of 67 / 67 / 66 outputs; ceil(200 / 64)
    assert a.tobytes() == b.tobytes() == c.tobytes() and ok_a.tolist() == ok_b.tolist() == [1] * 200
    want, _ = ic.expected(oracle, False, case)
    assert a.tobytes() == want.tobytes()


def test_indexed_harness_refuses_malformed_arguments(hc):
    z = np.zeros(64 * 32, dtype=np.uint8)
    p = z.ctypes.data
    for terms, n, P in ((0, 4, 1), (17, 4, 1), (1, 4, 0), (1, 4, 5), (1, 0, 1)):
        assert hc.hc_fb_indexed(0, p, 1, p, P, terms, p, n, 0, p, None, None) == -1
