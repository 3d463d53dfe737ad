"""The indexed fixed-base sums and LSSS share generation (include/gpbc_bn254_indexed.h), the part that needs no device: the new header
against _lib.INDEXED_SIGNATURES, the build's dependency lists, and the argument checks of the C entries and of the Python wrappers."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
import abi_headers
from gopairingbasedcryptography_amd import _build, _lib

VP, SZ = ctypes.c_void_p, ctypes.c_size_t
HEADER = os.path.join(ROOT, "include", "gpbc_bn254_indexed.h")


@pytest.fixture(scope="module")
def lib():
    _build.build_library()
    return _lib.load()


def test_indexed_signature_table_is_the_indexed_header(lib):
    protos = abi_headers.prototypes("gpbc_bn254_indexed.h")
    assert sorted(protos) == sorted(_lib.INDEXED_SIGNATURES) and len(protos) == 5
    assert len(_lib.SIGNATURES) == 131 and len(_lib.EXT_SIGNATURES) == 7
    ctype = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int}
    for name, (ret, params) in protos.items():
        assert _lib.INDEXED_SIGNATURES[name] == ret + ":" + "".join(params), name
        fn = getattr(lib, name)
        assert fn.restype is ctype[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [ctype[k] for k in params], name
    assert lib.gpbc_indexed_version() == 1
    assert (lib.gpbc_abi_version(), lib.gpbc_ext_version(), lib.gpbc_subset_version(), lib.gpbc_hash_version(), lib.gpbc_share_version()) == (8, 2, 1, 1, 1)
    header = open(HEADER).read()
    assert '#include "gpbc_bn254.h"' in header and "#define GPBC_INDEX_NONE 0xffffffffu" in header and "Entry map" in header


def test_build_lists_cover_the_new_header_and_lane_functions():
    assert "fbindex29.hip.hpp" in _build.HEADERS and "lsss29.hip.hpp" in _build.HEADERS
    assert 'include "fbindex29.hip.hpp"' in open(os.path.join(_build.CSRC, "gpbc_curve.hip")).read()
    assert 'include "lsss29.hip.hpp"' in open(os.path.join(_build.CSRC, "gpbc_fr.hip")).read()
    for h in ("fbindex29.hip.hpp", "lsss29.hip.hpp"):
        assert os.path.exists(os.path.join(_build.CSRC, h))


def test_c_entries_reject_invalid_share_arguments(lib):
    """GPBC_ERR_INVALID_ARG with a message, nothing written, before any device is touched; k = 0 is a no-op"""
    buf, out = np.zeros(64 * 64 * 32, np.uint8), np.zeros(64 * 32, np.uint8)
    p, o = VP(buf.ctypes.data), VP(out.ctypes.data)
    host, dev = lib.gpbc_fr_lsss_shares, lib.gpbc_fr_lsss_shares_dev
    bad = [
        (p, 1, 0, 1, p, 1, o, b"rows and cols"), (p, 1, 65, 1, p, 1, o, b"rows and cols"), (p, 1, 1, 0, p, 1, o, b"rows and cols"), (p, 1, 1, 65, p, 1, o, b"rows and cols"),
        (p, 1, 0, 1, p, 0, o, b"rows and cols"),                                           # an invalid shape is refused whatever k
        (p, 2, 4, 3, p, 3, o, b"n_matrices"), (p, 0, 4, 3, p, 3, o, b"n_matrices"), (p, 4, 4, 3, p, 3, o, b"n_matrices"),
        (None, 1, 4, 3, p, 1, o, b"null"), (p, 1, 4, 3, None, 1, o, b"null"), (p, 1, 4, 3, p, 1, None, b"null"),
        (p, 1, 4, 3, p, 1 << 29, o, b"too many"), (p, 1, 4, 3, p, (1 << 64) - 1, o, b"too many"),
        (p, 1, 4, 3, o, 2, VP(buf.ctypes.data + 11 * 32), b"overlaps"), (o, 1, 4, 3, p, 2, VP(out.ctypes.data + 7 * 32), b"overlaps"),
        (p, 2, 4, 3, o, 2, VP(buf.ctypes.data + 23 * 32), b"overlaps"),
    ]
    for a in bad:
        for fn, extra in ((host, []), (dev, [None])):
            rc = fn(a[0], SZ(a[1]), SZ(a[2]), SZ(a[3]), a[4], SZ(a[5]), a[6], *extra)
            assert rc == -1 and a[7] in lib.gpbc_last_error(), (a[1:6], lib.gpbc_last_error())
    assert host(None, SZ(1), SZ(4), SZ(3), None, SZ(0), None) == 0 and dev(None, SZ(1), SZ(4), SZ(3), None, SZ(0), None, None) == 0
    assert not out.any() and not buf.any()


def test_c_entries_reject_invalid_indexed_arguments(lib):
    """the size limits come first, then the handle: without a device there is no table, so a null handle stands in after the limits"""
    buf, out = np.zeros(64 * 32, np.uint8), np.zeros(64 * 128, np.uint8)
    p, o = VP(buf.ctypes.data), VP(out.ctypes.data)
    for fn, extra in ((lib.gpbc_fixed_base_indexed, []), (lib.gpbc_fixed_base_indexed_dev, [None])):
        for terms in (0, 17, (1 << 64) - 1):
            assert fn(None, p, SZ(1), SZ(terms), p, SZ(4), o, None, *extra) == -1 and b"terms" in lib.gpbc_last_error()
        assert fn(None, p, SZ(1), SZ(2), p, SZ(1 << 31), o, None, *extra) == -1 and b"2^32" in lib.gpbc_last_error()
        assert fn(None, p, SZ(1), SZ(1), p, SZ(1 << 32), o, None, *extra) == -1 and b"2^32" in lib.gpbc_last_error()
        assert fn(None, p, SZ(1), SZ(1), p, SZ(4), o, None, *extra) == -1 and b"null table" in lib.gpbc_last_error()
        assert fn(None, p, SZ(1), SZ(1), p, SZ(0), o, None, *extra) == -1                    # ... also for no outputs: there is no table to ask
    assert not out.any() and not buf.any()


class _FakeTable:
    """FixedBase without a device: the wrapper's own checks run before the C call"""
    def __new__(cls, nbase=3, g2=False):
        from gopairingbasedcryptography_amd import bn254
        t = bn254.FixedBase.__new__(bn254.FixedBase)
        t._lib, t.g2, t.width, t.nbase, t._h = None, g2, 128 if g2 else 64, nbase, ctypes.c_void_p()
        return t


def test_wrappers_reject_malformed_arguments():
    """ValueError before any C call (no device is touched: this runs without a GPU)"""
    import torch
    from gopairingbasedcryptography_amd import bn254
    z = lambda n: np.zeros(n, dtype=np.uint8)
    t = lambda n: torch.zeros(n, dtype=torch.uint8)
    f = bn254.fr_lsss_shares
    buf = z(24 * 32)
    bad = [
        lambda: f(z(12 * 32), z(3 * 32)),                                # bytes without rows / cols
        lambda: f(z(12 * 32), z(3 * 32), 4),
        lambda: f(z(12 * 32), z(3 * 32), 0, 3), lambda: f(z(12 * 32), z(3 * 32), 4, 0),
        lambda: f(z(65 * 32), z(32), 65, 1), lambda: f(z(65 * 32), z(65 * 32), 1, 65),
        lambda: f(z(13 * 32), z(3 * 32), 4, 3),                           # not whole matrices
        lambda: f(z(12 * 32), z(4 * 32), 4, 3),                           # not whole vectors
        lambda: f(z(24 * 32), z(9 * 32), 4, 3),                           # 2 matrices, 3 vectors
        lambda: f([[1, 2], [3]], [[1, 2]]),                               # ragged
        lambda: f([[1, 2], [3, 4]], [[1, 2, 3]]),
        lambda: f([[1 << 256, 2]], [[1, 2]]),                             # not a 32-byte value
        lambda: f(np.zeros(12 * 32, dtype=np.int8), z(3 * 32), 4, 3),     # dtype
        lambda: f(z(12 * 32), t(3 * 32), 4, 3),                           # host / device mix
        lambda: f(t(12 * 32), t(3 * 32), 4, 3),                           # host tensors: not CUDA
        lambda: f(z(12 * 32), z(6 * 32), 4, 3, out=z(4 * 32)),            # out too small (2 x 4)
        lambda: f(buf[:12 * 32], z(3 * 32), 4, 3, out=buf[11 * 32:15 * 32]),      # out overlaps the matrix
        lambda: f(z(12 * 32), buf[:3 * 32], 4, 3, out=buf[2 * 32:6 * 32]),        # out overlaps the vectors
    ]
    tab = _FakeTable()
    g = tab.indexed
    bad += [
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
        lambda: g(np.zeros(2, np.uint32), z(2 * 32), terms=1, out=z(64)),            # out too small
        lambda: g(np.zeros(2, np.uint32), z(2 * 32), terms=1),           # a closed table (no handle)
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    assert f(z(12 * 32), z(0), 4, 3).shape == (0, 4, 32)                 # no vectors: nothing to do, no device needed
    out, ok = g([[0, None]], z(0), terms=2)
    assert out.shape == (0, 64) and ok.shape == (0,)
    assert bn254.INDEX_NONE == 0xFFFFFFFF


def test_no_cpu_fallback_for_the_new_entries(lib):
    """without a GPU a valid call returns a negative status, writes nothing and leaves a message"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gopairingbasedcryptography_amd import bn254, EngineError
    out = np.zeros((1, 2, 32), np.uint8)
    with pytest.raises(EngineError):
        bn254.fr_lsss_shares([[1, 2], [3, 4]], [[5, 6]], out=out)
    m = np.zeros(4 * 32, np.uint8)
    p = lambda a: VP(a.ctypes.data)
    assert lib.gpbc_fr_lsss_shares(p(m), SZ(1), SZ(2), SZ(2), p(m), SZ(1), p(out)) < 0 and lib.gpbc_last_error()
    assert lib.gpbc_fr_lsss_shares_dev(p(m), SZ(1), SZ(2), SZ(2), p(m), SZ(1), p(out), None) < 0
    assert not out.any()
