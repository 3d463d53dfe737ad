"""The LSSS-weight kernel (csrc/fr29.hip.hpp: fr_lsss_*; csrc/gpbc_fr.hip: k_fr_lsss_weights), CPU part.

The lane functions of the kernel, compiled for the host with -DGPBC_BOUNDS (tools/bounds_check.cpp), against the elimination in
Python integers (lw11.reconstruction_weights), exactly: hc_fr_lsss_weights runs one system per wave, hc_fr_lsss_launch the launch
as it is made — geometry, staging into a checked stand-in for the LDS block, lane mapping, the ballots — workgroup by workgroup.
Every product in that build asserts its int64 columns and every canonical form its input range, so a run that finishes is the
overflow proof.  Then the wrapper's argument checks, the C entries' and the missing CPU fallback."""
import ctypes

import numpy as np
import pytest

from bounds_harness import hc  # noqa: F401  (the fixture)
import fr_cases as fc
import fr_lsss_cases as lc

VP, SZ = ctypes.c_void_p, ctypes.c_size_t
R = fc.R


def guarded(k, rows):
    """w with a guard row and ok with a guard byte behind them"""
    return np.full((k * rows + 1, 32), 0xA5, dtype=np.uint8), np.full(k + 1, 0xA5, dtype=np.uint8)


def hc_call(hc):
    def call(m, nm, rows, cols, held, k):
        w, ok = guarded(k, rows)
        assert hc.hc_fr_lsss_weights(m.ctypes.data, nm, rows, cols, held.ctypes.data, k, w.ctypes.data, ok.ctypes.data) == 0
        assert (w[k * rows] == 0xA5).all() and ok[k] == 0xA5
        return w[:k * rows], ok[:k]
    return call


def hc_launch(hc, geoms=None):
    def call(m, nm, rows, cols, held, k):
        w, ok = guarded(k, rows)
        geom = np.zeros(7, dtype=np.uint32)
        assert hc.hc_fr_lsss_launch(m.ctypes.data, nm, rows, cols, held.ctypes.data, k, w.ctypes.data, ok.ctypes.data, geom.ctypes.data) == 0
        assert (w[k * rows] == 0xA5).all() and ok[k] == 0xA5 and geom[6] == k * rows          # every weight has exactly one lane
        if geoms is not None:
            geoms.append(tuple(int(v) for v in geom[:6]))
        return w[:k * rows], ok[:k]
    return call


def test_case_lists_cover_what_they_claim():
    sizes = lc.size_cases()
    assert {(c["rows"], c["cols"]) for c in sizes} == set(lc.SIZES)
    assert {c["k"] for c in sizes + lc.large_k_cases()} >= set(lc.KS)
    for rows, cols in lc.SIZES:
        spw = lc.systems_per_workgroup(rows, cols)
        assert {c["k"] for c in sizes if (c["rows"], c["cols"]) == (rows, cols)} >= ({max(1, spw - 1), spw, spw + 1} if rows * cols < 63 * 63 else {1, 2})
    oks = {c["label"]: lc.expected(c)[1] for c in lc.policy_cases() + lc.pivot_cases() + lc.value_cases() + lc.dense_cases()}
    assert oks["and-or"] == [1, 1, 0, 1]
    w = lc.expected(lc.policy_cases()[0])[0]
    assert w[12:16] == [1, 1, 0, 0]                                       # all four held: rows 0 and 1 are used, the rest get 0
    for n in (1, 2, 16, 64):
        assert oks["and-chain-%d" % n][0] == 1 and not any(oks["and-chain-%d" % n][1:])
    assert oks["shamir-3-of-5"] == [1, 1, 1, 0, 0] and oks["shamir-8-of-16"] == [1, 1, 1, 0, 1]
    assert oks["nothing-held"] == [0] and oks["zero-matrix"] == [0]
    rep = lc.expected(lc.pivot_cases()[2])
    assert rep[1][0] == 1 and rep[0][:5] == [1, 1, 0, 1, 0]                # the second copy of a repeated row gets weight 0
    assert oks["r-where-the-pivot-search-looks"] == [1, 1, 1] and lc.expected(lc.value_cases()[2])[0][4:] == [0, 1]      # a row of multiples of r is a zero row
    assert oks["difference-zero"][0] == 1 and lc.expected(lc.value_cases()[3])[0][1] == 0
    assert oks["dense-8x8"] == [1] and oks["dense-64x64"] == [1]
    assert oks["dense-wide-5x9"] == [0] and oks["dense-wide-63x64"] == [0]  # rows < cols: the target is almost surely outside the span


def test_cases_under_bounds(hc):
    assert lc.run_cases(hc_call(hc), lc.all_cases()) == []


def test_cases_as_launched(hc):
    """every case through the launch geometry: no store or load outside a workgroup's staged systems, every weight written by one
    lane, Python's values; the sizes take the paths they are there for (group width, systems per workgroup, LDS instance)"""
    geoms = []
    assert lc.run_cases(hc_launch(hc, geoms), lc.all_cases()) == []
    by = {}
    for c, g in zip(lc.all_cases(), geoms):
        by.setdefault((c["rows"], c["cols"]), set()).add(g[:5])
        assert g[1] == lc.systems_per_workgroup(c["rows"], c["cols"]) and g[5] == -(-c["k"] // g[1])
    assert by[(16, 16)] == {(17, 3, 145, 2465, 0)} and by[(64, 64)] == {(64, 1, 577, 37505, 2)} and by[(63, 63)] == {(64, 1, 567, 36288, 2)}
    assert by[(3, 5)] == {(5, 12, 45, 180, 0)} and by[(1, 64)] == {(64, 1, 577, 1154, 0)} and by[(64, 1)] == {(64, 1, 9, 585, 0)}
    assert by[(1, 1)] == {(2, 32, 9, 18, 0)}


def test_ok_rows_satisfy_the_defining_identity(hc):
    for c in lc.policy_cases() + lc.pivot_cases() + lc.value_cases() + lc.broadcast_cases() + lc.dense_cases()[:1]:
        w, ok = hc_launch(hc)(lc.flat(c["matrices"]), len(c["matrices"]), c["rows"], c["cols"], lc.mask_bytes(c["held"]), c["k"])
        assert lc.satisfies(c, w, ok), c["label"]


def test_bound_margins_after_lsss(hc):
    st = np.zeros(7)
    lc.run_cases(hc_call(hc), lc.value_cases() + lc.dense_cases()[:1])
    hc.hc_stats(st.ctypes.data_as(VP))
    assert 0 < st[0] < 2.0**63 and st[1] < 2.0**31 and st[2] < 128


def test_harness_arguments(hc):
    z = np.zeros(64 * 64 * 32, dtype=np.uint8)
    p = z.ctypes.data
    for args in ((p, 1, 0, 1, p, 1), (p, 1, 1, 0, p, 1), (p, 1, 65, 1, p, 1), (p, 1, 1, 65, p, 1), (p, 2, 2, 2, p, 3), (None, 1, 2, 2, p, 1), (p, 1, 2, 2, None, 1)):
        assert hc.hc_fr_lsss_weights(*args, p, p) == -1 and hc.hc_fr_lsss_launch(*args, p, p, None) == -1, args


# ------------------------------------------------------------------------------------------------ the wrapper and the C entries
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


def test_wrapper_rejects_malformed_arguments():
    """ValueError before any C call (no device is touched: this runs without a GPU)"""
    import torch
    from gopairingbasedcryptography_amd import bn254
    z = lambda n: np.zeros(n, dtype=np.uint8)
    t = lambda n: torch.zeros(n, dtype=torch.uint8)
    f = bn254.fr_lsss_weights
    bad = [
        lambda: f(z(4 * 32), 2, 2),                                       # no mask
        lambda: f(z(4 * 32), 0, 2, z(2)),
        lambda: f(z(4 * 32), 2, 0, z(2)),
        lambda: f(z(65 * 32), 65, 1, z(65)),
        lambda: f(z(65 * 32), 1, 65, z(1)),
        lambda: f(z(4 * 32), None, 2, z(2)),                              # bytes without the shape
        lambda: f(z(5 * 32), 2, 2, z(2)),                                 # not whole matrices
        lambda: f(z(33), 1, 1, z(1)),
        lambda: f(z(2 * 4 * 32), 2, 2, z(6)),                             # 2 matrices, 3 masks
        lambda: f(z(3 * 4 * 32), 2, 2, z(4)),                             # 3 matrices, 2 masks
        lambda: f(z(4 * 32), 2, 2, z(3)),                                 # mask length
        lambda: f([[1, 2], [3]], held=[[1, 1]]),                          # ragged
        lambda: f([[1, 2], [3, 4]], held=[[1, 1, 1]]),
        lambda: f([[1 << 256, 2]], held=[[1]]),                           # not a 32-byte value
        lambda: f([[1, 2], [3, 4]], 3, 2, [[1, 1]]),                      # rows against the matrix
        lambda: f(np.zeros(4 * 32, dtype=np.int8), 2, 2, z(2)),           # dtype
        lambda: f(z(4 * 32), 2, 2, np.zeros(2, dtype=np.int32)),
        lambda: f(z(4 * 32), 2, 2, t(2)),                                 # host / device mix
        lambda: f(t(4 * 32), 2, 2, z(2)),
        lambda: f(t(4 * 32), 2, 2, t(2)),                                 # right sizes, but host tensors: not CUDA
        lambda: f(z(4 * 32), 2, 2, z(2), out=z(32)),                      # out too small
        lambda: f(z(4 * 32), 2, 2, z(2), ok_out=z(2)),
        lambda: f(z(4 * 32), 2, 2, z(2), out=np.zeros(64, dtype=np.int8)),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    w, ok = f(z(4 * 32), 2, 2, z(0))
    assert w.shape == (0, 2, 32) and ok.shape == (0,)                     # no masks: nothing to do, no device needed


def test_c_entries_reject_invalid_arguments(lib):
    """GPBC_ERR_INVALID_ARG with a message, nothing written, before any device is touched; k = 0 is a no-op"""
    buf, out = np.zeros(64 * 32, np.uint8), np.zeros(64 * 32, np.uint8)
    held, ok = np.ones(64, np.uint8), np.zeros(64, np.uint8)
    p, o, h, q = VP(buf.ctypes.data), VP(out.ctypes.data), VP(held.ctypes.data), VP(ok.ctypes.data)
    host, dev = lib.gpbc_fr_lsss_weights, lib.gpbc_fr_lsss_weights_dev
    for fn in (host, dev):
        fn.restype = ctypes.c_int
    bad = [
        (p, 1, 0, 2, h, 1, o, q, b"rows and cols"), (p, 1, 2, 0, h, 1, o, q, b"rows and cols"), (p, 1, 65, 1, h, 1, o, q, b"rows and cols"),
        (p, 1, 1, 65, h, 1, o, q, b"rows and cols"), (p, 2, 2, 2, h, 3, o, q, b"n_matrices"), (p, 0, 2, 2, h, 3, o, q, b"n_matrices"),
        (None, 1, 2, 2, h, 1, o, q, b"null"), (p, 1, 2, 2, None, 1, o, q, b"null"), (p, 1, 2, 2, h, 1, None, q, b"null"), (p, 1, 2, 2, h, 1, o, None, b"null"),
        (p, 1, 2, 2, h, 1 << 29, o, q, b"too many systems"), (p, 1, 2, 2, h, (1 << 64) - 1, o, q, b"too many systems"),
        (p, 1, 2, 2, h, 2, p, q, b"overlaps"), (p, 1, 2, 2, h, 2, VP(buf.ctypes.data + 3 * 32), q, b"overlaps"), (p, 1, 2, 2, h, 2, o, h, b"overlaps"),
        (p, 1, 2, 2, h, 2, o, VP(buf.ctypes.data + 5), b"overlaps"), (p, 1, 2, 2, h, 2, o, VP(out.ctypes.data + 127), b"overlaps"),
        (p, 1, 2, 2, h, 2, VP(held.ctypes.data), q, b"overlaps"),
    ]
    for a in bad:
        for fn, extra in ((host, []), (dev, [None])):
            rc = fn(a[0], SZ(a[1]), SZ(a[2]), SZ(a[3]), a[4], SZ(a[5]), a[6], a[7], *extra)
            assert rc == -1 and a[8] in lib.gpbc_last_error(), (a[1:6], lib.gpbc_last_error())
    assert host(None, SZ(1), SZ(2), SZ(2), None, SZ(0), None, None) == 0 and dev(None, SZ(1), SZ(2), SZ(2), None, SZ(0), None, None, None) == 0
    assert not out.any() and not buf.any() and not ok.any() and held.all()


def test_no_cpu_fallback_for_lsss(lib):
    """without a GPU a valid call returns a negative status, writes nothing and leaves a message"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gopairingbasedcryptography_amd import bn254, EngineError
    w, ok = np.zeros((1, 2, 32), np.uint8), np.zeros(1, np.uint8)
    with pytest.raises(EngineError):
        bn254.fr_lsss_weights([[1, 1], [0, R - 1]], held=[[1, 1]], out=w, ok_out=ok)
    m, h = fc.rows([1, 1, 0, R - 1]), np.ones(2, np.uint8)
    p = lambda a: VP(a.ctypes.data)
    assert lib.gpbc_fr_lsss_weights(p(m), SZ(1), SZ(2), SZ(2), p(h), SZ(1), p(w), p(ok)) < 0 and lib.gpbc_last_error()
    assert lib.gpbc_fr_lsss_weights_dev(p(m), SZ(1), SZ(2), SZ(2), p(h), SZ(1), p(w), p(ok), None) < 0
    assert not w.any() and not ok.any()
