"""Bit-selected sums over a fixed set (csrc/subset29.hip.hpp, csrc/gpbc_subset.hip, include/gpbc_bn254_subset.h), CPU part.

hc_subset_sum (tools/bounds_check.cpp) runs the table build, the chunk shape and the lane function of gpbc_subset_sum_dev on the host
with -DGPBC_BOUNDS against the oracle's point sum over [O] + the selected bases, byte for byte, on the case list of subset_cases.py.
A lane adds table rows into its accumulator window after window with no doubling in between; in that build every product asserts its
int64 columns and every table row its limb range, so a run that finishes is the overflow proof — the longest chain the cap allows for
one chunk (2 048 windows: 16 384 bits in a call that fills the chip) is among the cases.  Then the new header against
_lib.SUBSET_SIGNATURES, and the wrapper's and the C entries' argument checks, which need no device."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from bounds_harness import hc  # noqa: F401  (the fixture)
import abi_headers
import subset_cases as sc

VP, SZ = ctypes.c_void_p, ctypes.c_size_t
GROUPS = [False, True]
IDS = ["g1", "g2"]


def hc_run(hc, g2, t, masks=None, n_shape=0):
    masks = np.ascontiguousarray(t.masks if masks is None else masks, dtype=np.uint8)
    B = np.ascontiguousarray(t.B)
    O = None if t.O is None else np.ascontiguousarray(t.O)
    out = np.full((len(masks), sc.BYTES[g2]), 0xA5, dtype=np.uint8)
    hc.hc_subset_sum(int(g2), B.ctypes.data, t.nbits, None if O is None else O.ctypes.data, masks.ctypes.data, len(masks), n_shape, out.ctypes.data)
    return out


def shape(hc, W, n):
    v = (SZ * 4)()
    hc.hc_subset_shape(W, n, v)
    return list(v)


def test_shape_restated(hc):
    """the cap, and the chunks the cases aim at: one chunk up to 63 windows and for a call that fills the chip, at least 32 windows a chunk"""
    assert shape(hc, 32, 1)[:2] == [sc.MAX_BITS, 32]
    assert [shape(hc, W, 1)[2:] for W in (1, 32, 63, 64, 65, 256, 2048)] == [[1, 1], [1, 32], [1, 63], [2, 32], [2, 33], [8, 32], [64, 32]]
    assert shape(hc, 32, 1000)[2:] == [1, 32] and shape(hc, 256, 3)[2:] == [8, 32]
    assert shape(hc, 256, 1 << 16)[2:] == [2, 128] and shape(hc, 256, (1 << 16) + 1)[2:] == [2, 128] and shape(hc, 256, 1 << 17)[2:] == [1, 256]
    assert shape(hc, 2048, 131071)[2:] == [2, 1024] and shape(hc, 2048, 131072)[2:] == [1, 2048]
    for W in (64, 100, 257, 2048):
        for n in (1, 7, 5000, 70000):
            chunks, C = shape(hc, W, n)[2:]
            assert C >= 32 and (chunks - 1) * C < W <= chunks * C


@pytest.mark.parametrize("g2", GROUPS, ids=IDS)
def test_cases_under_bounds(hc, oracle, g2):
    """every table of the list against the oracle, byte for byte; a finished run is the overflow proof"""
    want = sc.expected(oracle, g2)
    ts = sc.tables(oracle, g2)
    assert len(ts) == len(sc.SIZES) * len(sc.SETS) * len(sc.OFFSETS)
    for t in ts:
        got = hc_run(hc, g2, t)
        bad = np.nonzero((got != want[t.label]).any(axis=1))[0]
        assert not len(bad), (t.label, [t.names[i] for i in bad[:8]])


@pytest.mark.parametrize("g2", GROUPS, ids=IDS)
def test_cases_reach_the_exceptional_additions(oracle, g2):
    """the expected bytes themselves say that the doubling cases end at 2P, the cancellation cases at infinity, and that the padding
    bits of the last byte change nothing"""
    want = {t.label: (t, sc.expected(oracle, g2)[t.label]) for t in sc.tables(oracle, g2)}
    P2 = sc.multiple(oracle, g2, 2 * 4242)
    for nbits in (9, 255, 256, 257, 2048):
        t, w = want["same/none/%d" % nbits]
        assert (w[t.row("0x80 0x80")] == P2).all()                                          # accumulator = entry: the doubling
        t, w = want["mirror/none/%d" % nbits]
        assert not w[t.row("0x80 0x80")].any() and w[t.row("0x80")].any()                    # accumulator = -entry: infinity
        if nbits > 16:
            assert (w[t.row("0x80 0x80, then 0x80")] == t.B[16]).all()                       # ... and on from infinity
        t, w = want["pairs/none/%d" % nbits]
        assert not w[t.row("0xC0")].any()                                                   # a table entry at infinity
        t, w = want["pairs/point/%d" % nbits]
        assert (w[t.row("0xC0")] == t.O).all() and t.O.any()
        t, w = want["rand/-B0/%d" % nbits]
        assert not w[t.row("0x80")].any() and (w[t.row("0xC0")] == t.B[1]).all()             # the offset cancels the entry
        t, w = want["holes/inf/%d" % nbits]
        assert not t.B[2].any() and not t.O.any() and w[t.row("ones")].any()
    for nbits in (1, 7, 9, 255, 257):
        for s in sc.SETS:
            t, w = want["%s/point/%d" % (s, nbits)]
            assert (t.masks[t.row("ones")] != t.masks[t.row("ones, padding clear")]).any()
            assert (w[t.row("ones")] == w[t.row("ones, padding clear")]).all()
            assert (w[t.row("padding bits only")] == w[t.row("zero")]).all() and (w[t.row("zero")] == t.O).all()
            assert (w[t.row("0x80 and the padding bits")] == w[t.row("0x80")]).all()
    t, w = want["rand/none/256"]
    assert (w[t.row("bit 0"):t.row("bit 0") + 256] == t.B).all() and not w[t.row("zero")].any()
    bits = np.unpackbits(np.frombuffer(__import__("hashlib").sha256(sc.DIGESTS[0].encode()).digest(), dtype=np.uint8))
    assert (np.unpackbits(t.masks[t.row("sha256 0")]) == bits).all() and 64 < bits.sum() < 192


@pytest.mark.parametrize("g2", GROUPS, ids=IDS)
def test_longest_chain_of_one_chunk(hc, oracle, g2):
    """16 384 bits in the shape of a call that fills the chip: ONE chunk, 2 048 additions in a row with no doubling between — all ones
    over distinct bases, all ones over one base (every window after the first meets a multiple of 8P), random masks"""
    nbits = sc.MAX_BITS
    assert shape(hc, nbits // 8, 131072)[2:] == [1, 2048]
    for s in ("rand", "same"):
        t = sc.make_table(oracle, g2, s, "point", nbits, extra_masks=sc.random_masks("chain" + s, 1, nbits // 8))
        rows = [t.row("ones"), t.row("extra 0"), t.row("sha256 1")]
        masks = t.masks[rows]
        assert (hc_run(hc, g2, t, masks, n_shape=131072) == sc.expect(oracle, g2, t, masks)).all(), s


def test_bound_margins_after_subset_sum(hc, oracle):
    t = sc.make_table(oracle, True, "rand", "point", 256)
    hc_run(hc, True, t)
    st = np.zeros(7)
    hc.hc_stats(st.ctypes.data_as(VP))
    assert 0 < st[0] < 2.0**63 and st[1] < 2.0**31


# ------------------------------------------------------------------------------------------------ the header, the wrapper, the C entries
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


def test_subset_signature_table_is_the_subset_header(lib):
    from gopairingbasedcryptography_amd import _lib
    protos = abi_headers.prototypes("gpbc_bn254_subset.h")
    assert sorted(protos) == sorted(_lib.SUBSET_SIGNATURES) and len(protos) == 9
    ctype = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int}
    for name, (ret, params) in protos.items():
        assert _lib.SUBSET_SIGNATURES[name] == ret + ":" + "".join(params), name
        fn = getattr(lib, name)
        assert fn.restype is ctype[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [ctype[k] for k in params], name
    assert lib.gpbc_subset_version() == 1 and lib.gpbc_abi_version() == 8 and lib.gpbc_ext_version() == 2
    assert '#include "gpbc_bn254.h"' in open(os.path.join(ROOT, "include", "gpbc_bn254_subset.h")).read()
    assert len(_lib.SIGNATURES) == 131 and len(_lib.EXT_SIGNATURES) == 7


def test_source_hash_covers_the_new_header_and_unit():
    from gopairingbasedcryptography_amd import _build
    assert "gpbc_subset.hip" in _build.UNITS and "subset29.hip.hpp" in _build.HEADERS


def test_table_bytes(lib):
    tb = lib.gpbc_subset_table_bytes
    assert tb(256, 1) == 32 * 256 * 257 == (2 << 20) + 8192 and tb(256, 0) == 32 * 256 * 129
    assert tb(1, 0) == tb(8, 0) == 256 * 129 and tb(9, 0) == 2 * 256 * 129
    assert tb(sc.MAX_BITS, 1) == 2048 * 256 * 257 and tb(sc.MAX_BITS + 1, 1) == 0 and tb(0, 0) == 0


def test_wrapper_rejects_malformed_arguments():
    """ValueError before any C call (no device is touched: this runs without a GPU)"""
    import torch
    from gopairingbasedcryptography_amd import bn254
    z = lambda *s: np.zeros(s, dtype=np.uint8)
    t = lambda *s: torch.zeros(s, dtype=torch.uint8)
    slots = bn254._slots
    for one, other, W in ((bn254.g1_subset_sum, bn254.g2_subset_sum, 64), (bn254.g2_subset_sum, bn254.g1_subset_sum, 128)):
        bad = [
            lambda: one(z(9, W), [[1, 2], [3]]),                                       # ragged masks
            lambda: one(z(9, W), z(2, 3)),                                             # wrong width: neither 2 bytes nor 9 bits
            lambda: one(z(9, W), z(2, 1)),
            lambda: one(z(9, W), z(4)),                                                # not two-dimensional
            lambda: one(z(9, W), np.full((2, 9), 2)),                                  # a bit array with other values
            lambda: one(z(9, W), np.array([[0, 1, 0, 1, 0, 1, 0, 1, -1]])),
            lambda: one(z(9, W), np.array([[0, 256]])),                                # bytes out of range
            lambda: one(z(9, W), np.array([[0.5, 1.0]])),
            lambda: one(z(9, W), z(2, 2), out=t(2, W)),                                # host / device mix
            lambda: one(z(9, W), t(2, 2)),
            lambda: one(t(9, W), z(2, 2)),
            lambda: one(z(9, W), z(2, 2), offset=t(W)),
            lambda: one(t(9, W), t(2, 2)),                                             # right kinds, but host tensors: not CUDA
            lambda: one(z(9, W), z(2, 2), out=z(3, W)),                                # wrong out
            lambda: one(z(9, W), z(2, 2), out=np.zeros((2, W), dtype=np.int8)),
            lambda: one(z(9, W), z(2, 2), out=z(2, 2 * W)[:, :W]),
            lambda: one(z(9 * W + 1), z(2, 2)),                                        # wrong point size
            lambda: one(z(9, 96), z(2, 2)) if W == 128 else one(z(9, 65), z(2, 2)),
            lambda: one(z(9, W), z(2, 2), offset=z(2, W)),
            lambda: one(z(9, W), z(2, 2), offset=z(W - 1)),
            lambda: one(z(0, W), z(2, 0)),                                             # no base
            lambda: one(z(sc.MAX_BITS + 1, W), z(1, sc.MAX_BITS // 8 + 1)),            # above the cap
            lambda: bn254.SubsetTable(z(9, W), g2=(W != 128)) if W == 64 else bn254.SubsetTable(z(3, 64), g2=True),
            lambda: bn254.SubsetTable(z(9, W), offset=z(2, W), g2=(W == 128)),
            lambda: bn254.SubsetTable(t(9, W), g2=(W == 128)),
        ]
        for i, call in enumerate(bad):
            with pytest.raises(ValueError):
                call()
            assert bn254._slots is slots, i


def test_c_entries_reject_invalid_arguments(lib):
    """GPBC_ERR_INVALID_ARG with a message, nothing written, before any device is touched"""
    p = lambda a: VP(a.ctypes.data)
    x, out = np.zeros(9 * 128, np.uint8), np.full(4 * 128, 0xA5, np.uint8)
    masks = np.zeros(8, np.uint8)
    for g2 in (0, 1):
        host = lib.gpbc_g2_subset_table_create if g2 else lib.gpbc_g1_subset_table_create
        h = VP(0x1234)
        bad = [lambda: host(p(x), 0, None, ctypes.byref(h)), lambda: host(p(x), sc.MAX_BITS + 1, None, ctypes.byref(h)), lambda: host(None, 9, None, ctypes.byref(h)),
               lambda: host(p(x), 9, None, None),
               lambda: lib.gpbc_subset_table_create_dev(g2, p(x), 0, None, None, ctypes.byref(h)),
               lambda: lib.gpbc_subset_table_create_dev(g2, p(x), sc.MAX_BITS + 1, None, None, ctypes.byref(h)),
               lambda: lib.gpbc_subset_table_create_dev(g2, None, 9, None, None, ctypes.byref(h)),
               lambda: lib.gpbc_subset_table_create_dev(g2, p(x), 9, None, None, None)]
        for i, call in enumerate(bad):
            h.value = 0x1234
            assert call() == -1 and lib.gpbc_last_error(), (g2, i)
            assert h.value in (None, 0) or i in (3, 7), (g2, i)                 # *out = NULL whenever there is an out
    assert b"cap" in (lib.gpbc_g1_subset_table_create(p(x), sc.MAX_BITS + 1, None, ctypes.byref(h)), lib.gpbc_last_error())[1]
    assert lib.gpbc_subset_sum(None, p(masks), 4, p(out)) == -1 and b"table" in lib.gpbc_last_error()
    assert lib.gpbc_subset_sum_dev(None, p(masks), 4, p(out), None, 0, None) == -1 and b"table" in lib.gpbc_last_error()
    assert lib.gpbc_subset_sum_workspace_bytes(None, 4) == 0 and lib.gpbc_subset_table_destroy(None) == 0
    assert (out == 0xA5).all() and not x.any()


def test_no_cpu_fallback_for_subset_sum(lib, oracle):
    """without a GPU a well-formed call returns a negative status and leaves a message"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gopairingbasedcryptography_amd import bn254, EngineError
    t = sc.make_table(oracle, False, "rand", "none", 9)
    with pytest.raises(EngineError):
        bn254.g1_subset_sum(t.B, t.masks)
    h = VP()
    assert lib.gpbc_g1_subset_table_create(VP(t.B.ctypes.data), 9, None, ctypes.byref(h)) < 0 and lib.gpbc_last_error() and not h.value
