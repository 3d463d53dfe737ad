"""Segmented inner products in Fr and GT.Equal (csrc/frdot29.hip.hpp with the entries in csrc/gpbc_fr.hip, k_gt_equal in
csrc/gpbc_pairing.hip, include/gpbc_bn254_verify.h), CPU part: the new header against _lib.VERIFY_SIGNATURES, the build's dependency
lists, every argument rejection of the C entries and of the Python wrappers (no device is needed), and the case list of
fr_dot_cases.py for what it claims to cover.  The kernels run in test_fr_dot_segments_gpu.py, the arithmetic on the host in
test_fr_dot_bounds.py."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
import abi_headers
import fr_dot_cases as fc

VP = ctypes.c_void_p
INVALID_ARG = -1
HEADER = os.path.join(ROOT, "include", "gpbc_bn254_verify.h")


# ------------------------------------------------------------------------------------------------ the case list
def test_case_list_covers_what_it_claims():
    assert fc.CASES["short"][0] == [0, 1, 2, 3, 63, 64, 65, 129]
    # G and G + 1 rounds in neighbouring wavefronts, without a cut ...
    ln = fc.CASES["g_and_g1"][0]
    assert fc.pieces(sum(ln), len(ln), True) == 1
    assert fc.launch_lanes(sum(ln), len(ln), True) == [64]
    r = [fc.rounds(v) for v in ln]
    assert any(b == a + 1 for a, b in zip(r, r[1:])) and any(b == a - 1 for a, b in zip(r, r[1:]))
    # ... and inside ONE wavefront, with 8 lanes per piece and with 32, where the wavefront's last piece slots are empty
    ln = fc.CASES["short_mixed"][0]
    assert fc.launch_lanes(sum(ln), len(ln), True) == [8] == fc.launch_lanes(sum(ln), len(ln), False) and len(ln) % 8 and len(ln) > 8
    r = [fc.rounds(v, 8) for v in ln[:8]]
    assert {0, 1, 2, 3} == set(r) and any(b == a + 1 for a, b in zip(r, r[1:]))
    ln = fc.CASES["short"][0]
    assert fc.launch_lanes(sum(ln), len(ln), True) == [32] and len({fc.rounds(v, 32) for v in ln[:2]}) == 2 and [fc.rounds(v, 32) for v in ln[6:]] == [2, 3]
    # ... and between the two pieces of one cut segment
    ln = fc.CASES["two_levels"][0]
    assert [j for j, _ in fc.levels(sum(ln), 1, True)] == [2, 1] == [j for j, _ in fc.levels(sum(ln), 1, False)]
    assert fc.launch_lanes(sum(ln), 1, True) == [64, 8]                                     # the fold of two values takes the narrowest pieces
    (p0, p1), = fc.piece_lengths(ln, 2)
    assert fc.rounds(p1) == fc.rounds(p0) + 1
    # three levels below 2^20 elements
    ln = fc.CASES["three_levels"][0]
    assert sum(ln) < 1 << 20 and [j for j, _ in fc.levels(sum(ln), 1, True)] == [1024, 2, 1] and len(fc.levels(sum(ln), 1, False)) == 3
    # a piece that is not cut and passes a reduction
    ln = fc.CASES["one_long_piece"][0]
    assert fc.pieces(sum(ln), len(ln), True) == 1 == fc.pieces(sum(ln), len(ln), False) and fc.rounds(ln[0]) > fc.RUN_MUL
    ln = fc.CASES["cut_uneven"][0]
    assert fc.pieces(sum(ln), len(ln), True) == 2 and 0 in ln and len(set(ln)) == 3
    for name in ("shared_short", "shared_cut"):
        assert "shared" in fc.case_modes(fc.CASES[name][0])
    assert fc.pieces(sum(fc.CASES["shared_cut"][0]), 2, True) == 2 and fc.pieces(sum(fc.CASES["shared_short"][0]), 5, True) == 1
    assert all(set(fc.case_modes(c[0])) >= {"dot", "sum"} for c in fc.CASES.values())
    assert fc.EXTREMES == {"r_minus_1": fc.R - 1, "all_ones": 2**256 - 1, "zero": 0}
    # n_seg x J <= fill + n_seg whatever the sizes
    for n, n_seg in ((1 << 20, 1), (1 << 20, 1 << 10), (1 << 20, 1 << 16), (5000, 3), (1 << 30, 5000)):
        for has_k in (True, False):
            assert n_seg * fc.pieces(n, n_seg, has_k) <= fc.FILL + n_seg


def test_case_constants_are_the_headers():
    text = open(os.path.join(ROOT, "gopairingbasedcryptography_amd", "csrc", "frdot29.hip.hpp")).read()
    assert "constexpr int FR_DOT_WAVE = %d;" % fc.WAVE in text and "constexpr int FR_DOT_LANES_MIN = %d;" % fc.LANES_MIN in text
    assert "FR_DOT_NORM = %d, FR_DOT_RUN_MUL = %d, FR_DOT_RUN_SUM = %d;" % (fc.NORM, fc.RUN_MUL, fc.RUN_SUM) in text
    assert "constexpr int FR_DOT_WAVES_PER_SIMD = 4;" in text and fc.FILL == 16 * 256 * 4 * 4
    assert "FR_DOT_SHAPE{16 * 256 * 4 * FR_DOT_WAVES_PER_SIMD, %d, %d};" % (fc.GROUP, fc.PLAIN_MIN) in text


def test_expectation_is_the_sum_of_products_mod_r():
    a, b = fc.rows_of([1, 2, 3, fc.R - 1, 2**256 - 1]), fc.rows_of([5, 6, 7, fc.R - 1, 2**256 - 1])
    seg = [0, 2, 2, 5]
    assert fc.ints(fc.expect(a, b, seg)) == [17, 0, (21 + 1 + (2**256 - 1) ** 2) % fc.R]
    assert fc.ints(fc.expect(a, None, seg)) == [3, 0, (3 + fc.R - 1 + 2**256 - 1) % fc.R]
    assert fc.ints(fc.expect(a[:4], b[:2], [0, 2, 4], shared=True)) == [17, (15 + 6 * (fc.R - 1)) % fc.R]
    assert fc.ints(fc.expect(a, b, [0, 2, 9], n=3)) == [17, 21]                              # offsets clamped to n


# ------------------------------------------------------------------------------------------------ the header, the tables, the build
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


def test_verify_signature_table_is_the_verify_header(lib):
    from gopairingbasedcryptography_amd import _lib
    protos = abi_headers.prototypes("gpbc_bn254_verify.h")
    assert sorted(protos) == sorted(_lib.VERIFY_SIGNATURES) == ["gpbc_fr_dot_segments", "gpbc_fr_dot_segments_dev", "gpbc_fr_dot_segments_workspace_bytes",
                                                                "gpbc_gt_equal", "gpbc_gt_equal_dev", "gpbc_verify_version"]
    ctype = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int}
    for name, (ret, params) in protos.items():
        assert _lib.VERIFY_SIGNATURES[name] == ret + ":" + "".join(params), name
        fn = getattr(lib, name)                                                            # load() declared it
        assert fn.restype is ctype[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [ctype[k] for k in params], name
    assert lib.gpbc_verify_version() == 1 and lib.gpbc_abi_version() == 8
    header = open(HEADER).read()
    assert '#include "gpbc_bn254.h"' in header
    assert all(cite in header for cite in ("bls_signature.go:71-89", "zss04_signature.go:337", "bb04_signature.go:292", "asbb.go:140"))


def test_build_lists_cover_the_new_files_and_no_new_unit():
    from gopairingbasedcryptography_amd import _build
    assert "frdot29.hip.hpp" in _build.HEADERS and os.path.exists(os.path.join(_build.CSRC, "frdot29.hip.hpp"))
    unit = open(os.path.join(_build.CSRC, "gpbc_fr.hip")).read()
    assert '#include "frdot29.hip.hpp"' in unit and "k_fr_dot_segments" in unit and "gpbc_bn254_verify.h" in unit
    assert "k_gt_equal" in open(os.path.join(_build.CSRC, "gpbc_pairing.hip")).read()


def test_workspace_plan(lib):
    """0 when no segment is cut; the piece values of the two parities, each padded to 256 bytes, otherwise"""
    pad = lambda b: (b + 255) // 256 * 256
    W = lib.gpbc_fr_dot_segments_workspace_bytes
    assert W(0, 0) == 0 and W(100, 1) == 0 and W(1 << 20, 1 << 16) == 0
    assert W(1025, 1) == pad(2 * 32)
    n = fc.CASES["three_levels"][0][0]
    assert W(n, 1) == pad(1024 * 32) + pad(2 * 32)
    assert W(1 << 20, 1 << 10) == pad((1 << 10) * 2 * 32)


# ------------------------------------------------------------------------------------------------ the C entries
def test_c_entries_reject_invalid_arguments(lib):
    """GPBC_ERR_INVALID_ARG with a message, nothing written, before any device is touched; n_seg == 0 / n == 0 are no-ops"""
    p = lambda a: VP(a.ctypes.data)
    a, b, out = np.zeros(6 * 32, np.uint8), np.zeros(6 * 32, np.uint8), np.full(2 * 32, 0xA5, np.uint8)
    seg, down, short, late = (np.array(v, dtype=np.uint64) for v in ([0, 2, 6], [0, 4, 3], [0, 3, 5], [1, 3, 6]))
    both = np.zeros(8 * 32, np.uint8)
    ws = np.zeros(1024, np.uint8)
    H, D = lib.gpbc_fr_dot_segments, lib.gpbc_fr_dot_segments_dev
    bad = [
        lambda: H(None, p(b), 6, p(seg), 2, p(out)),                                       # null a
        lambda: H(p(a), p(b), 6, None, 2, p(out)),                                         # null table
        lambda: H(p(a), p(b), 6, p(seg), 2, None),                                         # null out
        lambda: H(p(a), None, 6, p(seg), 2, p(out)),                                       # nb without b
        lambda: H(p(a), p(b), 5, p(seg), 2, p(out)),                                       # nb neither n nor n / n_seg
        lambda: H(p(a), p(b), 3, p(seg), 2, p(out)),                                       # a shared list of 3 over segments of 2 and 4
        lambda: H(p(a), p(b), 6, p(down), 2, p(out)),                                      # a table that decreases
        lambda: H(p(a), p(b), 6, p(late), 2, p(out)),                                      # ... that does not start at 0
        lambda: H(p(both), p(b), 6, p(seg), 2, VP(both.ctypes.data + 5 * 32)),             # out overlaps a
        lambda: H(p(a), p(both), 6, p(seg), 2, VP(both.ctypes.data + 5 * 32)),             # out overlaps b
        lambda: D(None, p(b), 6, p(seg), 6, 2, p(out), None, 0, None),
        lambda: D(p(a), p(b), 6, None, 6, 2, p(out), None, 0, None),
        lambda: D(p(a), p(b), 6, p(seg), 6, 2, None, None, 0, None),
        lambda: D(p(a), None, 6, p(seg), 6, 2, p(out), None, 0, None),
        lambda: D(p(a), p(b), 4, p(seg), 6, 2, p(out), None, 0, None),
        lambda: D(p(both), p(b), 6, p(seg), 6, 2, VP(both.ctypes.data + 5 * 32), None, 0, None),
        lambda: D(p(a), p(b), 1025, p(seg), 1025, 1, p(out), None, 0, None),               # a cut segment needs a workspace
        lambda: D(p(a), p(b), 1025, p(seg), 1025, 1, p(out), p(ws), 32, None),             # ... of the planned size
    ]
    for i, call in enumerate(bad):
        assert call() == INVALID_ARG and lib.gpbc_last_error(), i
    assert b"overlap" in (H(p(both), p(b), 6, p(seg), 2, VP(both.ctypes.data + 5 * 32)), lib.gpbc_last_error())[1]
    assert b"workspace" in (D(p(a), p(b), 1025, p(seg), 1025, 1, p(out), None, 0, None), lib.gpbc_last_error())[1]
    assert H(p(a), p(b), 6, p(short), 2, p(out)) == INVALID_ARG                             # (n = 5 from the table: nb = 6 fits nothing)
    assert (out == 0xA5).all() and not a.any() and not b.any()
    assert H(None, None, 0, None, 0, None) == 0 and D(None, None, 0, None, 0, 0, None, None, 0, None) == 0      # n_seg == 0: a no-op
    assert H(None, None, 7, p(down), 0, None) == 0
    # GT.Equal
    x, y, ok = np.zeros(3 * 384, np.uint8), np.zeros(3 * 384, np.uint8), np.full(3, 0xA5, np.uint8)
    E, ED = lib.gpbc_gt_equal, lib.gpbc_gt_equal_dev
    cat = np.zeros(3 * 384 + 3, np.uint8)
    bad = [
        lambda: E(None, p(y), 3, 3, p(ok)), lambda: E(p(x), None, 3, 3, p(ok)), lambda: E(p(x), p(y), 3, 3, None),
        lambda: E(p(x), p(y), 2, 3, p(ok)), lambda: E(p(x), p(y), 0, 3, p(ok)),
        lambda: E(p(cat), p(y), 3, 3, VP(cat.ctypes.data + 3 * 384 - 1)), lambda: E(p(x), p(cat), 1, 3, VP(cat.ctypes.data + 383)),
        lambda: ED(None, p(y), 3, 3, p(ok), None), lambda: ED(p(x), p(y), 2, 3, p(ok), None), lambda: ED(p(x), p(y), 3, 3, None, None),
        lambda: ED(p(x), p(cat), 1, 3, VP(cat.ctypes.data + 383), None),
    ]
    for i, call in enumerate(bad):
        assert call() == INVALID_ARG and lib.gpbc_last_error(), i
    assert (ok == 0xA5).all()
    assert E(None, None, 5, 0, None) == 0 and ED(None, None, 1, 0, None, None) == 0        # n == 0: nothing is looked at


def test_wrappers_reject_malformed_arguments():
    """ValueError before any C call (no device is touched: this runs without a GPU)"""
    import torch
    from gopairingbasedcryptography_amd import bn254
    z = lambda *s: np.zeros(s, dtype=np.uint8)
    t = lambda *s: torch.zeros(s, dtype=torch.uint8)
    slots = bn254._slots
    F, S, E = bn254.fr_dot_segments, bn254.fr_sum_segments, bn254.gt_equal
    bad = [
        lambda: F(z(6, 32), z(6, 32), [0, 2, 5]),                                          # the table does not end at n
        lambda: F(z(6, 32), z(6, 32), [1, 2, 6]),
        lambda: F(z(6, 32), z(6, 32), [0, 4, 3, 6]),
        lambda: F(z(6, 32), z(6, 32), [6]),                                                # no segment
        lambda: F(z(6, 32), z(5, 32), [0, 2, 6]),                                          # nb
        lambda: F(z(6, 32), z(3, 32), [0, 2, 6]),                                          # a shared list over unequal segments
        lambda: F(z(6, 31), z(6, 32), [0, 2, 6]),                                          # not whole rows
        lambda: F(z(6, 32), [1, 2, 3, 4, 5, 1 << 256], [0, 2, 6]),                         # integers out of range
        lambda: F([-1, 2], None, [0, 2]),
        lambda: F(z(6, 32), t(6, 32), [0, 2, 6]),                                          # kinds mixed
        lambda: F(t(6, 32), t(6, 32), [0, 2, 6]),                                          # host tensors: not CUDA
        lambda: F(z(6, 32), z(6, 32), [0, 2, 6], out=z(2, 31)),
        lambda: F(z(6, 32), z(6, 32), [0, 2, 6], out=t(2, 32)),
        lambda: S(z(6, 32), [0, 7]),
        lambda: E(z(3, 384), z(2, 384)),                                                   # neither one b nor one per a
        lambda: E(z(3, 384), z(0, 384)),
        lambda: E(z(3, 383), z(3, 383)),
        lambda: E(z(3, 384), t(3, 384)),
        lambda: E(z(3, 384), z(3, 384), out=z(4)),
        lambda: E(z(3, 384), z(3, 384), out=t(3)),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d was accepted" % i)
        assert bn254._slots is slots, i
    ok = E(z(0, 384), z(1, 384))                                                           # nothing to do: no engine call
    assert ok.shape == (0,) and ok.dtype == np.uint8 and bn254._slots is slots


def test_no_cpu_fallback(lib):
    """without a GPU a well-formed call returns a negative status and leaves a message; nothing is written"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gopairingbasedcryptography_amd import bn254, EngineError
    a, b, seg, _ = fc.case_inputs("short", "dot")
    with pytest.raises(EngineError):
        bn254.fr_dot_segments(a, b, seg)
    with pytest.raises(EngineError):
        bn254.fr_sum_segments(a, seg)
    with pytest.raises(EngineError):
        bn254.gt_equal(np.zeros((2, 384), np.uint8), np.zeros((1, 384), np.uint8))
    out = np.full(32, 0xA5, np.uint8)
    one = np.array([0, 1], dtype=np.uint64)
    assert lib.gpbc_fr_dot_segments(VP(a.ctypes.data), None, 0, VP(one.ctypes.data), 1, VP(out.ctypes.data)) < 0 and lib.gpbc_last_error()
    assert (out == 0xA5).all()
