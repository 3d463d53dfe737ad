"""Opening proofs over ragged batches on the CPU (include/gpbc_bn254_openings.h, csrc/openings29.hip.hpp, bn254.fr_poly_from_roots_segments,
bn254.FixedBase.openings):

  * the lane bodies of k_fr_poly_from_roots_segments and k_g1/g2_fb_openings compiled for the host with -DGPBC_BOUNDS (tools/bounds_check.cpp:
    hc_fr_poly_from_roots_segments, hc_fb_openings) over the corpus of tests/openings_cases.py against Python integers and the oracle's scalar
    multiplications and sums, with 1, 3 and 16 bases per lane.  Under GPBC_BOUNDS every product asserts its int64 columns and every
    normalisation its limbs, and a violation aborts: a run that finishes is the limb-bound proof for the Horner chain feeding the additions;
  * the header's prototypes against _lib.OPENINGS_SIGNATURES, that table loaded and disjoint from every other one, the version entry, the
    build lists;
  * the argument errors of the C entries (decided before any device is touched, nothing written) and of the Python wrappers."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT
from bounds_harness import hc  # noqa: F401  (the fixture)
import abi_headers
import openings_cases as oc

HEADER = os.path.join(ROOT, "include", "gpbc_bn254_openings.h")
SZ = ctypes.c_size_t
GUARD = 0xA5
R = oc.R


# ------------------------------------------------------------------------------------------------ the lane bodies
def roots_segments(hc, ids, counts, stride):
    seg, K = oc.segments(counts), oc.scalar_rows(ids)
    out = np.full(len(counts) * stride * 32 + 64, GUARD, dtype=np.uint8)
    assert hc.hc_fr_poly_from_roots_segments(K.ctypes.data if len(ids) else None, seg.ctypes.data, len(counts), stride, out.ctypes.data) == 0
    assert (out[len(counts) * stride * 32:] == GUARD).all()
    return out[:len(counts) * stride * 32]


def openings(hc, g2, ids, counts, C, with_ok=True, nbase=None):
    B = oc.bases(g2, nbase)
    nbase, width, n = B.shape[0], B.shape[1], len(ids)
    coeffs = oc.coeff_rows([v % R for v in ids], counts, nbase)
    seg, K = oc.segments(counts), oc.scalar_rows(ids)
    out, ok = np.full(n * width + 32, GUARD, dtype=np.uint8), np.full(n + 16, GUARD, dtype=np.uint8)
    rc = hc.hc_fb_openings(int(g2), B.ctypes.data, nbase, coeffs.ctypes.data, K.ctypes.data, seg.ctypes.data, len(counts), C, out.ctypes.data, ok.ctypes.data if with_ok else None)
    assert rc == 0
    assert (out[n * width:] == GUARD).all() and (ok[n if with_ok else 0:] == GUARD).all()
    return out[:n * width].reshape(n, width), ok[:n]


@pytest.mark.parametrize("nbase", [5, 9])
def test_batch_polynomials_over_ragged_segments(hc, nbase):
    """every segment length of the corpus in one call, rows of nbase scalars with zeros behind the coefficients; unreduced identities act
    as their residues; an empty segment is the polynomial 1"""
    ids, counts, names = oc.corpus(nbase)
    got = roots_segments(hc, ids, counts, nbase)
    assert got.tobytes() == oc.coeff_rows([v % R for v in ids], counts, nbase).tobytes()
    rows = got.reshape(len(counts), nbase, 32)
    for name in ("empty", "empty again"):
        assert rows[names.index(name), 0].tobytes() == (1).to_bytes(32, "little") and not rows[names.index(name), 1:].any()
    wide = roots_segments(hc, ids, counts, nbase + 7).reshape(len(counts), nbase + 7, 32)
    assert wide[:, :nbase].tobytes() == rows.tobytes() and not wide[:, nbase:].any()


def test_full_segments_give_the_bytes_of_the_uniform_kernel(hc):
    B, k = 7, 3
    ids = [oc.o.bench_scalar("openings_uniform", i) for i in range(B * k)]
    ids[4] = (1 << 256) - 1
    K = oc.scalar_rows(ids)
    old = np.zeros(k * (B + 1) * 32, dtype=np.uint8)
    assert hc.hc_fr_poly_from_roots(K.ctypes.data, B, k, old.ctypes.data) == 0
    assert roots_segments(hc, ids, [B] * k, B + 1).tobytes() == old.tobytes()


@pytest.mark.parametrize("C", [1, 3, 16])
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_openings_of_the_corpus(hc, oracle, g2, C):
    """chunks of 1, 3 and 16 bases per lane (16: one lane per identity, no sums to add, the lane masks its own row)"""
    ids, counts, names, want, want_ok, q = oc.expected_corpus(oracle, g2)
    nbase = oc.NBASE[g2]
    out, ok = openings(hc, g2, ids, counts, C)
    assert ok.tolist() == want_ok.tolist()
    assert not np.nonzero((out != want).any(1))[0].size
    B = oc.bases(g2)
    one, = oc.rows_of(counts, names, "one")
    assert q[one] == [1] and out[one].tobytes() == B[0].tobytes()                       # q = 1: the opening is base 0
    res = oc.rows_of(counts, names, "residues")
    assert ok[res].tolist() == [1, 1, 0, 0] and out[res[:2]].any(1).all() and not out[res[2:]].any()
    rep = oc.rows_of(counts, names, "repeated")
    assert ok[rep].tolist() == [0, 1, 0] and not out[rep[0]].any() and not out[rep[2]].any() and out[rep[1]].any()
    tau = oc.rows_of(counts, names, "tau")
    assert ok[tau].tolist() == [1, 1, 1] and not out[tau[0]].any() and not out[tau[2]].any() and out[tau[1]].any()
    assert all(out[i].any() and ok[i] for name in ("two", "three", "full") for i in oc.rows_of(counts, names, name))
    assert len(oc.rows_of(counts, names, "full")) == nbase - 1
    without_ok, _ = openings(hc, g2, ids, counts, C, with_ok=False)
    assert without_ok.tobytes() == want.tobytes()


def test_an_opening_is_the_quotient_at_tau(oracle):
    """the expectation itself, against a second statement: pi = [q(tau)] g, and the digest of the tau batch is infinity"""
    for g2 in (False, True):
        ids, counts, names, want, want_ok, q = oc.expected_corpus(oracle, g2)
        gen = oc.bases(g2)[0]
        mul = oracle.g2_scalar_mul if g2 else oracle.g1_scalar_mul
        live = [i for i in range(len(ids)) if want_ok[i]]
        at_tau = [sum(c * pow(oc.TAU, e, R) for e, c in enumerate(q[i])) % R for i in live]
        direct = np.asarray(mul(gen, oc.scalar_rows(at_tau))).reshape(len(live), -1)
        assert direct.tobytes() == want[live].tobytes()
        tau = oc.rows_of(counts, names, "tau")
        f = oc.poly_from_roots([ids[i] for i in tau])
        assert sum(c * pow(oc.TAU, e, R) for e, c in enumerate(f)) % R == 0 and at_tau[live.index(tau[1])] != 0


def test_the_chunk_rule_is_the_tables(hc):
    """opn_shape: one base per lane until 131072 lanes are busy, at most 16, never more than the table has"""
    def shape(nbase, n):
        out = (SZ * 2)()
        hc.hc_opn_shape(nbase, n, out)
        return tuple(out)
    assert shape(17, 54) == (1, 17) and shape(257, 2048) == (4, 65) and shape(257, 1 << 16) == (16, 17) and shape(5, 1 << 20) == (5, 1)
    assert shape(300, 302) == (1, 300)


def test_the_harness_refuses_what_the_entries_refuse(hc):
    K, out = np.zeros(2048 * 32, np.uint8), np.full(64, GUARD, np.uint8)
    seg = lambda *v: np.array(v, dtype=np.uint64)
    B = oc.bases(False)
    for s, k, stride in ((seg(0, 3, 2), 2, 9), (seg(1, 2), 1, 9), (seg(0, 9), 1, 9), (seg(0, 1025), 1, 2000), (seg(0, 1), 1, 0), (seg(0, 1), 1, (1 << 24) + 1)):
        assert hc.hc_fr_poly_from_roots_segments(K.ctypes.data, s.ctypes.data, k, stride, out.ctypes.data) == -1
    for s, k, C in ((seg(0, 3, 2), 2, 1), (seg(1, 2), 1, 1), (seg(0, 9), 1, 1), (seg(0, 2), 1, 0)):
        assert hc.hc_fb_openings(0, B.ctypes.data, 9, K.ctypes.data, K.ctypes.data, s.ctypes.data, k, C, out.ctypes.data, None) == -1
    assert hc.hc_fb_openings(0, B.ctypes.data, 9, K.ctypes.data, K.ctypes.data, seg(0, 0, 0).ctypes.data, 2, 1, out.ctypes.data, None) == 0
    assert (out == GUARD).all()


# ------------------------------------------------------------------------------------------------ the header, the table, the build
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


def test_signature_table_is_the_header_loaded_and_disjoint(lib):
    from gopairingbasedcryptography_amd import _lib
    protos = abi_headers.prototypes("gpbc_bn254_openings.h")
    mine = _lib.OPENINGS_SIGNATURES
    assert sorted(protos) == sorted(mine) == sorted(
        ["gpbc_openings_version", "gpbc_fr_poly_from_roots_segments", "gpbc_fr_poly_from_roots_segments_dev", "gpbc_fixed_base_openings_workspace_bytes",
         "gpbc_fixed_base_openings", "gpbc_fixed_base_openings_dev"])
    ctype = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int}
    for name, (ret, params) in protos.items():
        assert mine[name] == ret + ":" + "".join(params), name
        fn = getattr(lib, name)                                                            # load() declared it
        assert fn.restype is ctype[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [ctype[k] for k in params], name
    assert lib.gpbc_openings_version() == 1 and lib.gpbc_abi_version() == 8 and lib.gpbc_gtfixed_version() == 1
    header = open(HEADER).read()
    assert '#include "gpbc_bn254.h"' in header and "Entry map" in header
    assert all(cite in header for cite in ("gwww25_bibe.go:162-176", "afp25_bibe.go:293-305"))


def test_build_lists_name_the_new_unit_and_headers():
    from gopairingbasedcryptography_amd import _build
    assert "gpbc_openings.hip" in _build.UNITS and "openings29.hip.hpp" in _build.HEADERS
    for f in ("gpbc_openings.hip", "openings29.hip.hpp"):
        assert os.path.exists(os.path.join(_build.CSRC, f))
    unit = open(os.path.join(_build.CSRC, "gpbc_openings.hip")).read()
    assert all(k in unit for k in ("k_g1_fb_openings", "k_g2_fb_openings", "k_fr_poly_from_roots_segments", '#include "openings29.hip.hpp"'))
    for older in ("gpbc_curve.hip", "gpbc_fr.hip"):
        assert "openings" not in open(os.path.join(_build.CSRC, older)).read(), older
    assert "openings29.hip.hpp" in open(os.path.join(ROOT, "tools", "bounds_check.cpp")).read()


class FakeHandle(ctypes.Structure):
    """gpbc_fixed_base as csrc/gpbc_curve.hip lays it out, with no table behind it: enough for the checks that come before any device.
    Only calls that are refused on their arguments are made with it."""
    _fields_ = [("device", ctypes.c_int), ("is_g2", ctypes.c_int), ("nbase", ctypes.c_size_t), ("table", ctypes.c_void_p), ("base_inf", ctypes.c_void_p)]


def test_c_argument_errors_come_before_any_device(lib):
    buf, out, ok = np.zeros(4096 * 32, np.uint8), np.full(64 * 64, GUARD, np.uint8), np.full(64, GUARD, np.uint8)
    p, o, k = buf.ctypes.data, out.ctypes.data, ok.ctypes.data
    seg = lambda *v: np.array(v, dtype=np.uint64)
    err = lambda: lib.gpbc_last_error()
    for fn, extra in ((lib.gpbc_fr_poly_from_roots_segments, []), (lib.gpbc_fr_poly_from_roots_segments_dev, [None])):
        call = lambda s, kk, stride, roots=p, dst=o: fn(roots, s.ctypes.data if s is not None else None, kk, stride, dst, *extra)
        assert call(seg(0, 3, 2), 2, 8) == -1 and b"monotone" in err()                      # a decreasing table
        assert call(seg(1, 3), 1, 8) == -1 and b"seg_off[0]" in err()
        assert call(seg(0, 8), 1, 8) == -1 and b"stride - 1" in err()                       # m + 1 > stride
        assert call(seg(0, 1025), 1, 4096) == -1 and b"FR_POLY_MAX_B" in err()              # m > 1024
        assert call(seg(0, 1), 1, 0) == -1 and call(seg(0, 1), 1, (1 << 24) + 1) == -1 and b"stride" in err()
        assert call(None, 1, 8) == -1 and b"null segment table" in err()
        assert call(seg(0, 2), 1, 8, roots=None) == -1 and call(seg(0, 2), 1, 8, dst=None) == -1 and b"null pointer" in err()
        assert call(seg(0, 2), 1, 8, dst=p + 32) == -1 and b"overlaps" in err()
        assert call(seg(0, 2), 1 << 31, 8) == -1 and b"too many" in err()
        assert call(seg(0, 2), 0, 8, roots=None, dst=None) == 0                              # k == 0: a no-op
    h = FakeHandle(0, 0, 9, None, None)
    hp = ctypes.addressof(h)
    for fn, extra in ((lib.gpbc_fixed_base_openings, []), (lib.gpbc_fixed_base_openings_dev, [None, 0, None])):
        def call(s, kk, handle=hp, coeffs=p, ids=p + 9 * 32 * 4, dst=o, flags=k):
            return fn(handle, coeffs, ids, s.ctypes.data if s is not None else None, kk, dst, flags, *extra)
        assert call(seg(0, 2), 1, handle=None) == -1 and b"null table" in err()
        assert call(seg(0, 2), 0, handle=None) == -1 and call(seg(0, 2), 0) == 0
        assert call(seg(0, 3, 2), 2) == -1 and b"monotone" in err()
        assert call(seg(1, 3), 1) == -1 and call(None, 1) == -1
        assert call(seg(0, 9), 1) == -1 and b"nbase - 1" in err()                           # m + 1 > nbase: the rows do not fit the table
        for bad in (dict(coeffs=None), dict(ids=None), dict(dst=None)):
            assert call(seg(0, 2), 1, **bad) == -1 and b"null pointer" in err()
        # coeffs at p (one row of 9 scalars), the two identities behind them: an output reaching into either, and ok_out inside out
        for bad in (dict(dst=p + 32), dict(dst=p + 9 * 32 * 4 + 63), dict(flags=p + 9 * 32 - 1), dict(flags=p + 9 * 32 * 4), dict(flags=o + 127), dict(ids=o + 64)):
            assert call(seg(0, 2), 1, **bad) == -1 and b"overlaps" in err(), bad
        assert call(seg(0, 0, 0), 2, coeffs=None, ids=None, dst=None) == 0                   # no identities: nothing to do
    big = FakeHandle(0, 1, 2000, None, None)
    assert lib.gpbc_fixed_base_openings(ctypes.addressof(big), p, p, seg(0, 1025).ctypes.data, 1, o, None) == -1 and b"FR_POLY_MAX_B" in err()
    # a table of 257 bases at 2048 identities adds 65 chunks: the workspace is asked for before any device, too
    wide = FakeHandle(0, 0, 257, None, None)
    need = lib.gpbc_fixed_base_openings_workspace_bytes(ctypes.addressof(wide), 2048)
    assert need >= (65 + 5) * 2048 * 64 + 2048 and lib.gpbc_fixed_base_openings_workspace_bytes(hp, 54) >= 9 * 54 * 64 + 54
    one = FakeHandle(0, 0, 1, None, None)                                                    # one chunk: nothing to add, no workspace
    assert lib.gpbc_fixed_base_openings_workspace_bytes(ctypes.addressof(one), 54) == 0 and lib.gpbc_fixed_base_openings_workspace_bytes(None, 5) == 0
    big_seg = np.arange(0, 2049, 256, dtype=np.uint64)
    huge, wide_out = np.zeros(8 * 257 * 32, np.uint8), np.full(2048 * 64, GUARD, np.uint8)
    assert lib.gpbc_fixed_base_openings_dev(ctypes.addressof(wide), huge.ctypes.data, p, big_seg.ctypes.data, 8, wide_out.ctypes.data, None, None, 0, None) == -4
    assert b"workspace" in err() and (wide_out == GUARD).all()
    assert (out == GUARD).all() and (ok == GUARD).all() and not buf.any()


class _FakeTable:
    """FixedBase without a device: the wrapper's own checks run before the C call"""
    def __new__(cls, nbase=9, handle=None, g2=False):
        from gopairingbasedcryptography_amd import bn254
        t = bn254.FixedBase.__new__(bn254.FixedBase)
        t._lib, t.nbase, t._h, t.g2, t.width = None, nbase, ctypes.c_void_p(handle), g2, 128 if g2 else 64
        return t


def test_python_argument_errors():
    """ValueError before any C call (no device is touched: this runs without a GPU)"""
    import torch
    from gopairingbasedcryptography_amd import bn254
    assert list(inspect.signature(bn254.fr_poly_from_roots_segments).parameters) == ["roots", "counts", "stride", "out"]
    assert list(inspect.signature(bn254.FixedBase.openings).parameters) == ["self", "ids", "counts", "coeffs", "out", "ok_out"]
    z = lambda n: np.zeros(n, dtype=np.uint8)
    t = lambda n: torch.zeros(n, dtype=torch.uint8)
    buf = z(64 * 32)
    f, g = bn254.fr_poly_from_roots_segments, _FakeTable(handle=0x1000).openings
    bad = [
        lambda: f([1, 2, 3], [2, 2], 4), lambda: f([1, 2, 3], 2, 4),                     # the segments do not hold the roots
        lambda: f([1, 2, 3], [3], 3), lambda: f([1, 2, 3], [4, -1], 8),                  # m + 1 > stride; a negative length
        lambda: f(z(1025 * 32), [1025], 2000),                                           # m > 1024
        lambda: f([1, 2], [2], 0), lambda: f([1, 2], [2], (1 << 24) + 1), lambda: f([1, 2], [2], 3.0), lambda: f([1, 2], [2], True),
        lambda: f([1, 2], "ab", 4), lambda: f([1, 2], 0, 4),
        lambda: f([1 << 256], [1], 4), lambda: f(z(33), [1], 4),
        lambda: f(z(64), [2], 4, out=z(4 * 32 - 1)), lambda: f(z(64), [2], 4, out=t(4 * 32)),
        lambda: f(buf[:64], [2], 4, out=buf[32:32 + 128]),                               # out overlaps the roots
        lambda: g([1, 2, 3], [2, 2]), lambda: g([1, 2, 3], 2),
        lambda: g(list(range(9)), [9]),                                                  # m + 1 > nbase: a stride mismatch with the table
        lambda: g([1, 2], [2], coeffs=z(8 * 32)), lambda: g([1, 2], [1, 1], coeffs=z(9 * 32)),       # coeffs rows are nbase scalars, one per batch
        lambda: g([1, 2], [2], coeffs=t(9 * 32)),                                        # host / device mix
        lambda: g([1, 2], [2], out=z(64)), lambda: g([1, 2], [2], ok_out=z(3)), lambda: g([1, 2], [2], ok_out=np.zeros(2, np.int32)),
        lambda: g(buf[:64], [2], out=buf[32:32 + 128]), lambda: g(buf[:64], [2], coeffs=buf[64:64 + 9 * 32], ok_out=buf[64:66]),
        lambda: _FakeTable().openings([1, 2], [2]),                                      # a closed table
        lambda: _FakeTable(nbase=2000, handle=0x1000).openings(z(1025 * 32), [1025]),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert not buf.any(), i
    out, ok = _FakeTable().openings([], [0, 0])                                          # no identities: nothing to do, no device needed
    assert out.shape == (0, 64) and ok.shape == (0,)
    assert _FakeTable(g2=True).openings(z(0), [])[0].shape == (0, 128)
