"""Fixed-base exponentiation in GT on the CPU (include/gpbc_bn254_gtfixed.h, csrc/gtfixed29.hip.hpp, bn254.GTFixedBase):

  * the lane bodies of k_gt_fb_build and k_gt_fb_indexed compiled for the host with -DGPBC_BOUNDS (tools/bounds_check.cpp: hc_gt_fb_build,
    hc_gt_fb_indexed) over the corpus of tests/gt_fixed_cases.py against Python integers.  Under GPBC_BOUNDS every product asserts its int64
    columns and every normalisation its limbs, for the interval classes of the operands, and a violation aborts: a run that finishes is the
    limb-bound proof for the chain f12p_mul(output of f12p_mul, normalised table entry), for bases outside the cyclotomic subgroup and zero
    included;
  * the header's prototypes against _lib.GTFIXED_SIGNATURES and that table loaded, the version entries, the build lists;
  * the argument errors of the C entries (decided before any device is touched, nothing written) and of the Python class."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT
from bounds_harness import hc  # noqa: F401  (the fixture)
import abi_headers
import gt_fixed_cases as gc

HEADER = os.path.join(ROOT, "include", "gpbc_bn254_gtfixed.h")
VP = ctypes.c_void_p
GUARD = 0xA5
NBASE = 4
TABLE_DWORDS = 1 << 20                                                 # 4 MiB of int32 per base


# ------------------------------------------------------------------------------------------------ the lane bodies
@pytest.fixture(scope="module")
def table(hc):
    """the tables of one, e(g1, g2), a Miller value and zero, built once by the build kernel's lane body, with guards behind them"""
    t = np.full(NBASE * TABLE_DWORDS + 64, 0x5A5A5A5A, dtype=np.int32)
    B = gc.bases()
    assert hc.hc_gt_fb_build(B.ctypes.data, NBASE, t.ctypes.data) == 0
    assert (t[NBASE * TABLE_DWORDS:] == 0x5A5A5A5A).all()
    return t


def indexed(hc, table, nbase, index, scalars, n, with_ok=True):
    terms = len(index[0])
    idx, K = gc.index_array(index), gc.scalar_rows([k for row in scalars for k in row])
    out, ok = np.full(n * 384 + 32, GUARD, dtype=np.uint8), np.full(n + 16, GUARD, dtype=np.uint8)
    assert hc.hc_gt_fb_indexed(table.ctypes.data, nbase, idx.ctypes.data, len(index), terms, K.ctypes.data, n, out.ctypes.data, ok.ctypes.data if with_ok else None) == 0
    assert (out[n * 384:] == GUARD).all() and (ok[n if with_ok else 0:] == GUARD).all()
    return out[:n * 384].reshape(n, 384), ok[:n]


def test_table_entries_are_the_powers(table):
    """entry (j, w, d) in the layout of f6_row_store, C0's half-row and then C1's: d = 0 is one in every window of every base, every
    positive power of zero is zero, the padding dwords of every half-row are zero, and the limbs below the top one are normalised (what
    f6_row_load declares of a table entry)"""
    rows = table[:NBASE * TABLE_DWORDS].reshape(NBASE, 32, 256, 2, 64)
    assert not rows[..., 54:56].any() and (rows[..., 56:] == 0x5A5A5A5A).all()                 # 14 quads written per half-row, the rest left alone
    one_even = rows[gc.PAIRING, 0, 0, 0, :54]
    assert one_even.any() and (rows[:, :, 0, 0, :54] == one_even).all() and not rows[:, :, 0, 1, :54].any()      # C0 = 1, C1 = 0
    assert not rows[gc.ZERO, :, 1:, :, :54].any()
    low = rows[..., :54].reshape(NBASE, 32, 256, 2, 6, 9)[..., :8]
    assert (low >= 0).all() and (low < 1 << 29).all()


@pytest.mark.parametrize("nbase", [1, NBASE])
def test_every_exponent_on_every_base(hc, table, nbase):
    index, scalars, n = gc.every_base_every_exponent(nbase)
    want, want_ok = gc.expected(index, scalars, n, nbase)
    out, ok = indexed(hc, table, nbase, index, scalars, n)
    assert ok.tolist() == want_ok.tolist() and not np.nonzero((out != want).any(1))[0].size
    if nbase == NBASE:
        from gopairingbasedcryptography_amd._plan import GT_ONE
        E = len(gc.EXPONENTS)
        assert out[gc.ZERO * E].tobytes() == GT_ONE.tobytes() and not out[gc.ZERO * E + 1:].any()
        assert out[gc.PAIRING * E + gc.EXPONENTS.index(gc.o.R)].tobytes() == GT_ONE.tobytes()
        assert out[gc.MILLER * E + gc.EXPONENTS.index(gc.o.R)].tobytes() != GT_ONE.tobytes()


@pytest.mark.parametrize("n,terms,rows", [(9, 1, 9), (9, 2, 9), (7, 16, 7), (5, 2, 1), (7, 3, 3)])
def test_terms_special_rows_and_periodic_rows(hc, table, n, terms, rows):
    """1, 2 and 16 terms (the longest chain: 512 products), own and periodic index rows; with own rows the row of only INDEX_NONE, the row
    with an index equal to nbase (zero, ok = 0, neighbours untouched) and the row of one base under k and r - k"""
    from gopairingbasedcryptography_amd._plan import GT_ONE
    index, scalars = gc.shaped(n, terms, rows, NBASE)
    want, want_ok = gc.expected(index, scalars, n, NBASE)
    out, ok = indexed(hc, table, NBASE, index, scalars, n)
    assert ok.tolist() == want_ok.tolist() and out.tobytes() == want.tobytes()
    if rows == n:
        assert out[1].tobytes() == GT_ONE.tobytes() and ok.tolist() == [1, 1, 1, 0] + [1] * (n - 4) and not out[3].any() and out[2].any() and out[4].any()
        if terms >= 2:
            assert out[5].tobytes() == GT_ONE.tobytes() and index[5][:2] == [gc.PAIRING, gc.PAIRING]
    without_ok, _ = indexed(hc, table, NBASE, index, scalars, n, with_ok=False)
    assert without_ok.tobytes() == want.tobytes()


def test_the_harness_refuses_what_the_entry_refuses(hc, table):
    K, idx, out = np.zeros(17 * 32, np.uint8), np.zeros(17, np.uint32), np.full(384, GUARD, np.uint8)
    for nrows, terms, n in ((1, 0, 1), (1, 17, 1), (0, 1, 1), (2, 1, 1), (1, 2, 1 << 31)):
        assert hc.hc_gt_fb_indexed(table.ctypes.data, NBASE, idx.ctypes.data, nrows, terms, K.ctypes.data, n, out.ctypes.data, None) == -1
    assert hc.hc_gt_fb_indexed(table.ctypes.data, NBASE, idx.ctypes.data, 1, 1, K.ctypes.data, 0, out.ctypes.data, None) == 0
    assert (out == GUARD).all()


# ------------------------------------------------------------------------------------------------ the header, the table, the build
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


def test_signature_table_is_the_header_loaded_and_disjoint(lib):
    """the new table is what the header declares, and load() has declared it"""
    from gopairingbasedcryptography_amd import _lib
    protos = abi_headers.prototypes("gpbc_bn254_gtfixed.h")
    mine = _lib.GTFIXED_SIGNATURES
    assert sorted(protos) == sorted(mine) == sorted(
        ["gpbc_gtfixed_version", "gpbc_gt_fixed_base_table_bytes", "gpbc_gt_fixed_base_create", "gpbc_gt_fixed_base_create_dev", "gpbc_gt_fixed_base_destroy",
         "gpbc_gt_fixed_base_indexed", "gpbc_gt_fixed_base_indexed_dev"])
    ctype = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int}
    for name, (ret, params) in protos.items():
        assert mine[name] == ret + ":" + "".join(params), name
        fn = getattr(lib, name)                                                            # load() declared it
        assert fn.restype is ctype[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [ctype[k] for k in params], name
    assert lib.gpbc_gtfixed_version() == 1 and lib.gpbc_abi_version() == 8
    assert lib.gpbc_gt_fixed_base_table_bytes(1) == 4 << 20 and lib.gpbc_gt_fixed_base_table_bytes(16) == 64 << 20
    assert lib.gpbc_gt_fixed_base_table_bytes(0) == 0 and lib.gpbc_gt_fixed_base_table_bytes((1 << 64) - 1) == 0
    header = open(HEADER).read()
    assert '#include "gpbc_bn254.h"' in header and "Entry map" in header
    assert all(cite in header for cite in ("bb04_sibe.go:195-200", "bb04_ibe.go:181-189", "waters05_ibe.go:214"))


def test_build_lists_name_the_new_unit_and_headers():
    from gopairingbasedcryptography_amd import _build
    assert "gpbc_gtfixed.hip" in _build.UNITS and "gtfixed29.hip.hpp" in _build.HEADERS
    for f in ("gpbc_gtfixed.hip", "gtfixed29.hip.hpp"):
        assert os.path.exists(os.path.join(_build.CSRC, f))
    unit = open(os.path.join(_build.CSRC, "gpbc_gtfixed.hip")).read()
    assert all(k in unit for k in ("k_gt_fb_build", "k_gt_fb_indexed", '#include "gtfixed29.hip.hpp"'))
    for older in ("gpbc_pairing.hip", "gpbc_gtmexp.hip"):
        assert "gt_fb_" not in open(os.path.join(_build.CSRC, older)).read(), older


def test_c_argument_errors_come_before_any_device(lib):
    """the limits, the pointers and their ranges are decided on the arguments alone, and the handle last: without a device there is no
    table, so a null handle stands in and is itself refused where everything else is in order — also for n = 0"""
    buf, out, ok = np.zeros(64 * 32, np.uint8), np.full(4 * 384, GUARD, np.uint8), np.full(4, GUARD, np.uint8)
    p, o, k = buf.ctypes.data, out.ctypes.data, ok.ctypes.data
    for fn, extra in ((lib.gpbc_gt_fixed_base_indexed, []), (lib.gpbc_gt_fixed_base_indexed_dev, [None])):
        def call(index, nrows, terms, scalars, n, out_, ok_):
            return fn(None, index, nrows, terms, scalars, n, out_, ok_, *extra)
        for terms in (0, 17, (1 << 64) - 1):
            assert call(p, 1, terms, p, 4, o, None) == -1 and b"terms" in lib.gpbc_last_error()
        assert call(p, 1, 2, p, 1 << 31, o, None) == -1 and b"2^32" in lib.gpbc_last_error()
        assert call(p, 1, 1, p, 1 << 32, o, None) == -1 and b"2^32" in lib.gpbc_last_error()
        for nrows in (0, 5):
            assert call(p, nrows, 1, p, 4, o, None) == -1 and b"n_index_rows" in lib.gpbc_last_error()
        for args in ((None, 4, 1, p, 4, o, k), (p, 4, 1, None, 4, o, k), (p, 4, 1, p, 4, None, k)):
            assert call(*args) == -1 and b"null pointer" in lib.gpbc_last_error()
        # scalars at p (4 x 32 bytes), index behind them: out or ok_out reaching into either, and ok_out inside out
        for args in ((p + 128, 4, 1, p, 4, p + 127, None), (p + 128, 4, 1, p, 4, p + 143, None), (p + 128, 4, 1, p, 4, o, p + 127), (p + 128, 4, 1, p, 4, o, p + 143),
                     (p + 128, 4, 1, p, 4, o, o + 4 * 384 - 1), (o + 4 * 384 - 16, 4, 1, p, 4, o, None)):
            assert call(*args) == -1 and b"overlaps" in lib.gpbc_last_error(), args
        assert call(p + 128, 4, 1, p, 4, o, k) == -1 and b"null table" in lib.gpbc_last_error()
        assert call(p, 1, 1, p, 0, o, k) == -1 and b"null table" in lib.gpbc_last_error()
    h = VP()
    for fn, extra in ((lib.gpbc_gt_fixed_base_create, []), (lib.gpbc_gt_fixed_base_create_dev, [None])):
        h.value = 0x1234
        assert fn(p, 0, *extra, ctypes.byref(h)) == -1 and b"at least one base" in lib.gpbc_last_error() and not h.value
        assert fn(None, 1, *extra, ctypes.byref(h)) == -1 and fn(p, 1, *extra, None) == -1
        assert fn(p, 1 << 24, *extra, ctypes.byref(h)) == -1 and b"too many" in lib.gpbc_last_error()
    assert lib.gpbc_gt_fixed_base_destroy(None) == 0
    assert (out == GUARD).all() and (ok == GUARD).all() and not buf.any()


class _FakeTable:
    """GTFixedBase without a device: the wrapper's own checks run before the C call"""
    def __new__(cls, nbase=3, handle=None):
        from gopairingbasedcryptography_amd import bn254
        t = bn254.GTFixedBase.__new__(bn254.GTFixedBase)
        t._lib, t.nbase, t._h, t._rows = None, nbase, ctypes.c_void_p(handle), {}
        return t


def test_python_argument_errors():
    """ValueError before any C call (no device is touched: this runs without a GPU)"""
    import torch
    from gopairingbasedcryptography_amd import bn254
    assert list(inspect.signature(bn254.GTFixedBase.__init__).parameters) == ["self", "bases"]
    assert list(inspect.signature(bn254.GTFixedBase.pow).parameters) == ["self", "scalars", "base", "out"]
    assert list(inspect.signature(bn254.GTFixedBase.indexed).parameters) == ["self", "index", "scalars", "terms", "out", "ok_out"]
    assert all(hasattr(bn254.GTFixedBase, m) for m in ("table_bytes", "close"))
    z = lambda n: np.zeros(n, dtype=np.uint8)
    t = lambda n: torch.zeros(n, dtype=torch.uint8)
    tab, buf = _FakeTable(handle=0x1000), z(4 * 384)
    g, pw = tab.indexed, tab.pow
    bad = [
        lambda: g(np.zeros(2, np.uint32), z(2 * 32)),                    # an array without terms
        lambda: g(np.zeros(2, np.uint32), z(2 * 32), terms=0), lambda: g(np.zeros(17, np.uint32), z(17 * 32), terms=17),
        lambda: g([[0] * 17], [[1] * 17]),
        lambda: g(np.zeros(2, np.int64), z(2 * 32), terms=1),            # dtype
        lambda: g(np.zeros(0, np.uint32), z(2 * 32), terms=1),           # n_index_rows 0
        lambda: g(np.zeros(3, np.uint32), z(2 * 32), terms=1),           # n_index_rows n + 1
        lambda: g(np.zeros(3, np.uint32), z(4 * 32), terms=2),           # not whole index rows
        lambda: g(np.zeros(2, np.uint32), z(3 * 32), terms=2),           # not whole scalar rows
        lambda: g([[0, 1], [2]], [[1, 2], [3, 4]]),                      # ragged
        lambda: g([[0, -1]], [[1, 2]]), lambda: g([[0, 1 << 32]], [[1, 2]]),
        lambda: g([[0, 1]], [[1, 1 << 256]]),
        lambda: g(np.zeros(2, np.uint32), t(2 * 32), terms=1),           # host / device mix
        lambda: g(np.zeros(2, np.uint32), z(2 * 32), terms=1, out=z(384)),                       # out too small
        lambda: g(np.zeros(2, np.uint32), z(2 * 32), terms=1, ok_out=z(3)),                      # ok_out too large
        lambda: g(np.zeros(2, np.uint32), z(2 * 32), terms=1, ok_out=np.zeros(2, np.int32)),     # ... of the wrong dtype
        lambda: g(np.zeros(2, np.uint32), buf[:64], terms=1, out=buf[32:32 + 768]),              # out overlaps the scalars
        lambda: g(np.zeros(2, np.uint32), buf[:64], terms=1, ok_out=buf[63:65]),                 # ok_out overlaps the scalars
        lambda: pw([1, 2], base=3), lambda: pw([1, 2], base=-1), lambda: pw([1, 2], base=True), lambda: pw([1, 2], base=0.0),
        lambda: pw([1 << 256]),
        lambda: _FakeTable().pow([1, 2]),                                # a closed table (no handle)
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert not buf.any(), i
    out, ok = _FakeTable().indexed([[0, None]], z(0), terms=2)          # no outputs: nothing to do, no device needed
    assert out.shape == (0, 384) and ok.shape == (0,)
    assert _FakeTable().pow(z(0)).shape == (0, 384)
