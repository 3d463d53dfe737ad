"""Elementwise group law: G1 / G2 addition, subtraction and doubling of affine points (csrc/group29.hip.hpp, csrc/gpbc_group.hip).

CPU: the lane function of the kernels, compiled for the host with -DGPBC_BOUNDS (tools/bounds_check.cpp, hc_group_op: the same
grouping of K elements per shared inversion), against the Python oracle bit for bit — random pairs, every special case at every
position of an inversion group and in a group of nothing but special cases, a broadcast b, sizes 1, K-1, K+1 and 1000.  A run
that finishes is also the overflow proof of the formulas.  Argument checks and the missing CPU fallback through the wrapper.

GPU: the same cases through the host and the device entries, in place included; a 2^20 algebraic check against the engine's
scalar multiplication (independent of the new kernels); a ZSS04 verification and BSW07 key components kept in HBM."""
import ctypes

import numpy as np
import pytest

import bn254_py as o  # noqa: F401
from bounds_harness import hc  # noqa: F401  (the fixture)
from group_law_cases import ADD, DBL, GROUPS, OPS, SPECIALS, SUB, group_k, make_special, run_hc, special_batch



# ------------------------------------------------------------------------------------------------ CPU: the harness
@pytest.mark.parametrize("name", ["g1", "g2"])
@pytest.mark.parametrize("op", OPS)
def test_random_pairs_under_bounds(hc, oracle, name, op):
    """random pairs for n in {1, K-1, K+1, 1000}: the kernels' lane function on the host equals the oracle bit for bit"""
    grp = GROUPS[name]
    K = group_k(hc, grp)
    for n in (1, K - 1, K + 1, 1000):
        A, B = grp.points(oracle, "grp-a%d-%d" % (op, n), n), grp.points(oracle, "grp-b%d-%d" % (op, n), n)
        got = run_hc(hc, grp, op, A, None if op == DBL else B)
        want = grp.expect(op, A, B)
        assert (got == want).all(), (name, op, n, np.nonzero((got != want).any(axis=1))[0][:8])


SPECIAL_CASES = [(op, kind) for op in (ADD, SUB) for kind in SPECIALS] + [(DBL, "a_inf")]


@pytest.mark.parametrize("name", ["g1", "g2"])
@pytest.mark.parametrize("op,kind", SPECIAL_CASES)
def test_special_cases_at_every_group_position(hc, oracle, name, op, kind):
    """inf inputs, a = b, a = -b (and a - a, DBL inf) at every position 0 .. K-1 of one inversion group, and a group of nothing
    but that case: the result is the oracle's, and the neighbours in the group are not spoiled"""
    grp = GROUPS[name]
    K = group_k(hc, grp)
    A, B = special_batch(grp, oracle, op, kind, K, "sp-%s-%d-%s" % (name, op, kind))
    got = run_hc(hc, grp, op, A, None if op == DBL else B)
    want = grp.expect(op, A, B)
    assert (got == want).all(), (name, op, kind, np.nonzero((got != want).any(axis=1))[0][:8])


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_broadcast_b_under_bounds(hc, oracle, name):
    """nb = 1: one b for every a (a public key added to every [H(m_i)]g2); a holds b, -b and infinity at a few places, and a
    broadcast b at infinity returns a (ADD, SUB)"""
    grp = GROUPS[name]
    K = group_k(hc, grp)
    n = 5 * K + 3
    A = grp.points(oracle, "bc-a-" + name, n)
    B = grp.points(oracle, "bc-b-" + name, 1)
    A[3] = B[0]
    A[K + 1] = grp.neg_rows(B)[0]
    A[2 * K] = 0
    for op in (ADD, SUB):
        got = run_hc(hc, grp, op, A, B)
        assert (got == grp.expect(op, A, B)).all(), (name, op)
        Z = np.zeros_like(B)
        got = run_hc(hc, grp, op, A, Z)
        assert (got == grp.expect(op, A, Z)).all(), (name, op, "b = inf")


def test_group_sizes_under_bounds(hc, oracle):
    """the shared-inversion walk is correct for any group size the harness can instantiate (1, 4, 6, 8; 0 = the kernels' K)"""
    for name in ("g1", "g2"):
        grp = GROUPS[name]
        n = 37
        A, B = grp.points(oracle, "gs-a-" + name, n), grp.points(oracle, "gs-b-" + name, n)
        make_special(grp, "a_eq_b", A, B, 5)
        make_special(grp, "a_eq_neg_b", A, B, 6)
        make_special(grp, "b_inf", A, B, 17)
        want = grp.expect(ADD, A, B)
        for k in (1, 4, 6, 8, 0):
            assert (run_hc(hc, grp, ADD, A, B, k) == want).all(), (name, k)


def test_bound_margins_after_group_law(hc, oracle):
    """the worst column / limb / value seen over the group-law runs stays inside int64 / int32 / the lazy-reduction budget"""
    grp = GROUPS["g2"]
    A, B = grp.points(oracle, "bm-a", 16), grp.points(oracle, "bm-b", 16)
    for op in OPS:
        run_hc(hc, grp, op, A, None if op == DBL else B)
    st = np.zeros(7)
    hc.hc_stats(st.ctypes.data_as(ctypes.c_void_p))
    assert 0 < st[0] < 2.0**63 and st[1] < 2.0**31 and st[2] < 128


# ------------------------------------------------------------------------------------------------ CPU: the wrapper and the C entries
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


ENTRIES = [("g1", 64, "add"), ("g1", 64, "sub"), ("g2", 128, "add"), ("g2", 128, "sub")]


def test_invalid_arguments_rejected(lib):
    """nb outside {1, n} and null pointers: GPBC_ERR_INVALID_ARG with a message from the C entries (EngineError through the
    wrapper's check), ValueError from the wrapper's own shape checks — before any device is touched"""
    from gopairingbasedcryptography_amd import _lib, bn254, EngineError
    vp = ctypes.c_void_p
    for g, w, op in ENTRIES:
        a, b, out = np.zeros(5 * w, np.uint8), np.zeros(3 * w, np.uint8), np.zeros(5 * w, np.uint8)
        host = getattr(lib, "gpbc_%s_%s_batch" % (g, op))
        dev = getattr(lib, "gpbc_%s_%s_batch_dev" % (g, op))
        for rc in (host(vp(a.ctypes.data), vp(b.ctypes.data), ctypes.c_size_t(3), ctypes.c_size_t(5), vp(out.ctypes.data)),
                   host(None, vp(b.ctypes.data), ctypes.c_size_t(1), ctypes.c_size_t(5), vp(out.ctypes.data)),
                   host(vp(a.ctypes.data), None, ctypes.c_size_t(5), ctypes.c_size_t(5), vp(out.ctypes.data)),
                   host(vp(a.ctypes.data), vp(b.ctypes.data), ctypes.c_size_t(5), ctypes.c_size_t(5), None),
                   dev(vp(a.ctypes.data), vp(b.ctypes.data), ctypes.c_size_t(2), ctypes.c_size_t(5), vp(out.ctypes.data), None),
                   dev(None, vp(b.ctypes.data), ctypes.c_size_t(1), ctypes.c_size_t(5), vp(out.ctypes.data), None)):
            assert rc == -1 and lib.gpbc_last_error()
            with pytest.raises(EngineError):
                _lib.check(rc)
        assert not out.any()
        fn = getattr(bn254, "%s_%s" % (g, op))
        with pytest.raises(ValueError):
            fn(a, b)                                                 # 3 b for 5 a
        with pytest.raises(ValueError):
            fn(a, b, out=np.zeros(4 * w, np.uint8))                  # out of the wrong size
    for g, w in (("g1", 64), ("g2", 128)):
        out = np.zeros(4 * w, np.uint8)
        assert getattr(lib, "gpbc_%s_double_batch" % g)(None, ctypes.c_size_t(4), vp(out.ctypes.data)) == -1
        assert getattr(lib, "gpbc_%s_double_batch_dev" % g)(vp(out.ctypes.data), ctypes.c_size_t(4), None, None) == -1
        assert getattr(lib, "gpbc_%s_add_batch" % g)(None, None, ctypes.c_size_t(0), ctypes.c_size_t(0), None) == 0   # n = 0: nothing to do
        with pytest.raises(ValueError):
            getattr(bn254, "%s_double" % g)(np.zeros(w + 1, np.uint8))


def test_no_cpu_fallback_for_group_law(lib):
    """without a GPU every new entry raises and leaves the output untouched"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gopairingbasedcryptography_amd import bn254, EngineError
    g1, g2 = bn254.generators()
    for name, g in (("g1", g1), ("g2", g2)):
        a = np.tile(g, 3)
        for op in ("add", "sub"):
            out = np.zeros(a.size, np.uint8)
            with pytest.raises(EngineError):
                getattr(bn254, "%s_%s" % (name, op))(a, g, out=out)
            assert not out.any()
        out = np.zeros(a.size, np.uint8)
        with pytest.raises(EngineError):
            getattr(bn254, "%s_double" % name)(a, out=out)
        assert not out.any()
        rc = getattr(lib, "gpbc_%s_add_batch" % name)(a.ctypes.data_as(ctypes.c_void_p), g.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(1),
                                                       ctypes.c_size_t(3), out.ctypes.data_as(ctypes.c_void_p))
        assert rc < 0 and not out.any()
