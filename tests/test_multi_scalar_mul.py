"""Segmented G1 / G2 multi-scalar multiplication (csrc/gmsm29.hip.hpp, csrc/gpbc_gmsm.hip, include/gpbc_bn254_ext.h), CPU part.

hc_multi_scalar_mul (tools/bounds_check.cpp) runs the plan and the lane functions of gpbc_g*_multi_scalar_mul_dev on the host with
-DGPBC_BOUNDS — the same piece cut, the same gmsm_lane / gmsm_sum_lane per lane, the same folds — against the oracle's scalar
multiplication summed per segment, bit for bit, on the case lists of gmsm_cases.py.  The loop adds rescaled table rows into the
accumulator up to GMSM_GROUP times in a row with no doubling between and adds group results with jac_add: in that build every product
asserts its int64 columns and every table row its limb range, so a run that finishes is the overflow proof.  Then the wrapper's and the
C entries' argument checks, which need no device, and the extension header against _lib.EXT_SIGNATURES."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from bounds_harness import hc  # noqa: F401  (the fixture)
import abi_headers
import gmsm_cases as gc

VP = ctypes.c_void_p
GROUPS = [False, True]
IDS = ["g1", "g2"]


def hc_run(hc, g2, x, k, seg):
    w = gc.BYTES[g2]
    x = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, w)
    kr = gc.krows(k) if k is not None and len(k) else np.zeros((1, 32), dtype=np.uint8)
    s = np.array(seg, dtype=np.uint64)
    out = np.full((len(seg) - 1, w), 0xA5, dtype=np.uint8)
    hc.hc_multi_scalar_mul(int(g2), x.ctypes.data if len(x) else None, kr.ctypes.data if k is not None else None, len(k) if k is not None else 0,
                           s.ctypes.data, len(x), len(seg) - 1, out.ctypes.data)
    return out


def test_plan_restated(hc):
    """the cut the case lists aim at: J from the sizes alone, and the boundaries named in gmsm_cases"""
    for g2 in GROUPS:
        G = gc.group(g2)
        assert G == hc.hc_gmsm_group(int(g2)) and 1 <= G <= 8
        assert [gc.pieces(L, 1, True, g2) for L in (0, 1, 2 * G - 1, 2 * G, 2 * G + 1, 3 * G - 1, 3 * G, 16 * G - 1, 16 * G, 16 * G + 1)] == [1, 1, 1, 2, 2, 2, 3, 15, 16, 16]
        assert [gc.pieces(L, 1, False, g2) for L in (15, 16, 17, 127, 128, 129, 1023, 1024)] == [1, 2, 2, 15, 16, 16, 127, 128]
        # fold levels of one segment: J pieces are folded as a plain sum of J points
        levels = lambda L, has_k: 0 if gc.pieces(L, 1, has_k, g2) == 1 else 1 + levels(gc.pieces(L, 1, has_k, g2), False)
        assert [levels(L, True) for L in (2 * G - 1, 2 * G, 16 * G - 1, 16 * G, 128 * G - 1, 128 * G)] == [0, 1, 1, 2, 2, 3]
        assert [levels(L, False) for L in (15, 16, 127, 128, 1023, 1024, 8191, 8192)] == [0, 1, 1, 2, 2, 3, 3, 4]
        assert levels(sum(gc.lengths_with_scalars(g2)) // (len(gc.lengths_with_scalars(g2)) + 2), True) >= 2        # the combined call folds twice
        assert gc.pieces(1 << 20, 1, False, g2) == 131072 and gc.pieces(1 << 20, 1 << 16, True, g2) == min(16 // G, 2) and gc.pieces(1 << 20, 1 << 17, True, g2) == 1
        assert gc.pieces(1 << 18, 1 << 12, True, g2) == min(64 // G, 32)


@pytest.mark.parametrize("g2", GROUPS, ids=IDS)
def test_cases_under_bounds(hc, oracle, g2):
    """every case of the list against the oracle, bit for bit; a finished run is the overflow proof"""
    want = gc.expected(oracle, g2)
    seen = set()
    for label, x, k, seg, shared in gc.cases(g2):
        got = hc_run(hc, g2, x, k, seg)
        assert (got == want[label]).all(), (label, np.nonzero((got != want[label]).any(axis=1))[0][:8])
        seen.add(label)
    assert len(seen) > 60
    if not g2:
        # what a device-resident table can do: the last offset lies past n.  The kernels' own segment range clamps every offset to n:
        # 6 points, table [0, 4, 9] -> out[1] is the sum over x[4:6], and nothing past x[5] is read (x and k hold exactly 6 rows)
        x, k = gc.take(gc.pool(g2)["pt"], 6), gc.rand_scalars("past-n", 6)
        assert (hc_run(hc, g2, x, k, [0, 4, 9]) == gc.expect(oracle, g2, x, k, [0, 4, 6], False)).all()


def test_cases_reach_the_exceptional_additions(oracle):
    """the expected bytes themselves say that the cancellation cases end at infinity and the doubling case at 2P"""
    for g2 in GROUPS:
        want, p = gc.expected(oracle, g2), gc.pool(g2)
        assert all("segments of " + name in want for name in ("G, G + 1", "G + 1, G", "G, 2G", "G, G, G + 1"))
        for label in ("P - P by the scalar", "P + (-P), equal scalars", "2 P - 2P"):
            assert not want[label].any() and not want[label + ", across a group boundary"].any(), label
        assert (want["P + P"][0] == p["dbl"][0]).all() and (want["P + P, across a group boundary"][0] == p["dbl"][0]).all()
        assert want["infinity mid-segment, then more terms"].any() and not want["infinity alone"].any()


def test_digit_scalars_cover_the_window_positions(hc):
    """the scalars of gmsm_cases.digit_scalars put a non-zero digit into every window of the GLV halves (two-bit windows 0 .. 62 of k1
    and of k2) and into every bit 0 .. 63 of the four GLS quarters, as the splits themselves report"""
    k = gc.krows(gc.digit_scalars(False))
    rows = np.zeros((len(k), 12), dtype=np.uint32)
    hc.hc_glv_split(k.ctypes.data, len(k), rows.ctypes.data)
    for half in (0, 5):
        v = [sum(int(r[half + i]) << (32 * i) for i in range(5)) for r in rows]
        assert all(any((x >> (2 * w)) & 3 for x in v) for w in range(63)), half
    k = gc.krows(gc.digit_scalars(True))
    rows = np.zeros((len(k), 16), dtype=np.uint32)
    hc.hc_gls_split(k.ctypes.data, len(k), rows.ctypes.data)
    for q in range(4):
        v = [sum(int(r[4 * q + i]) << (32 * i) for i in range(3)) for r in rows]       # rows: [magnitude (3 x u32), sign] per quarter
        assert all(any((x >> w) & 1 for x in v) for w in range(64)), q


@pytest.mark.parametrize("g2", GROUPS, ids=IDS)
def test_one_term_segments_are_the_scalar_multiplication(hc, oracle, g2):
    """segments of one term are ScalarMultiplication itself, for the harness form of k_g*_scalar_mul too (hc_g1_mul / hc_g2_mul)"""
    p = gc.pool(g2)
    ks = gc.EDGE_SCALARS + gc.rand_scalars("single", 7)
    x = np.concatenate([gc.take(p["pt"], len(ks) - 1), p["inf"]])
    got = hc_run(hc, g2, x, ks, list(range(len(ks) + 1)))
    ref = np.zeros_like(got)
    (hc.hc_g2_mul if g2 else hc.hc_g1_mul)(np.ascontiguousarray(x).ctypes.data, gc.krows(ks).ctypes.data, len(ks), ref.ctypes.data)
    assert (got == ref).all() and (got == gc.expect(oracle, g2, x, ks, list(range(len(ks) + 1)), False)).all()


def test_bound_margins_after_multi_scalar_mul(hc):
    p = gc.pool(False)
    G = gc.group(False)
    hc_run(hc, False, gc.take(p["pt"], 2 * G + 1), gc.rand_scalars("bm", 2 * G + 1), [0, 2 * G + 1])
    st = np.zeros(7)
    hc.hc_stats(st.ctypes.data_as(VP))
    assert 0 < st[0] < 2.0**63 and st[1] < 2.0**31


# ------------------------------------------------------------------------------------------------ the wrapper and the C entries
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


def test_ext_signature_table_is_the_extension_header(lib):
    """every prototype of the extension header is what _lib.EXT_SIGNATURES declares, load() has set restype and argtypes from it,
    and the main table does not hold the new names (it mirrors the main header alone)"""
    from gopairingbasedcryptography_amd import _lib
    protos = abi_headers.prototypes("gpbc_bn254_ext.h")
    assert sorted(protos) == sorted(_lib.EXT_SIGNATURES) and len(protos) == 7
    ctype = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int}
    for name, (ret, params) in protos.items():
        assert _lib.EXT_SIGNATURES[name] == ret + ":" + "".join(params), name
        fn = getattr(lib, name)
        assert fn.restype is ctype[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [ctype[k] for k in params], name
    assert lib.gpbc_ext_version() == 2 and lib.gpbc_abi_version() == 8
    assert '#include "gpbc_bn254.h"' in open(os.path.join(ROOT, "include", "gpbc_bn254_ext.h")).read()


def test_small_call_stats_symbol_and_signature(lib):
    """revision 2 of the extension header: four uint64_t out-pointers, an int status, declared in EXT_SIGNATURES and wrapped as a tuple"""
    from gopairingbasedcryptography_amd import _lib, bn254
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "gpbc_bn254_ext.h")).read())
    assert ("int gpbc_small_call_stats(uint64_t *batches_out, uint64_t *calls_out, uint64_t *largest_batch_out, "
            "uint64_t *failed_in_shared_batches_out);") in text
    assert _lib.EXT_SIGNATURES["gpbc_small_call_stats"] == "i:pppp" and abi_headers.prototypes("gpbc_bn254_ext.h")["gpbc_small_call_stats"] == ("i", ["p"] * 4)
    fn = lib.gpbc_small_call_stats
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == [ctypes.c_void_p] * 4
    v = [ctypes.c_uint64(1 << 63) for _ in range(4)]
    assert fn(*(ctypes.byref(x) for x in v)) == 0
    got = bn254.small_call_stats()
    assert isinstance(got, tuple) and len(got) == 4 and all(isinstance(x, int) for x in got)
    # counters only grow, and a batch holds at least one call and at most all of them
    assert all(a.value <= b for a, b in zip(v, got)) and got[0] <= got[1] and got[2] <= got[1] and got[3] <= got[1]


def test_small_call_stats_are_zero_before_any_call():
    """a fresh process that loads the library and binds no device: all four counters are zero, and stay zero after a small call that is
    refused for want of a device (nothing was batched).  A process of its own, because the counters are process-wide since load."""
    import subprocess
    import sys
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    prog = ("import ctypes, sys\n"
            "lib = ctypes.CDLL(sys.argv[1])\n"
            "v = [ctypes.c_uint64(7) for _ in range(4)]\n"
            "rc = [lib.gpbc_small_call_stats(*(ctypes.byref(x) for x in v))]\n"
            "first = [x.value for x in v]\n"
            "P, Q, out = ctypes.create_string_buffer(64), ctypes.create_string_buffer(128), ctypes.create_string_buffer(384)\n"
            "lib.gpbc_pair_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]\n"
            "rc.append(lib.gpbc_pair_batch(P, Q, 1, out))\n"
            "rc.append(lib.gpbc_small_call_stats(*(ctypes.byref(x) for x in v)))\n"
            "print(rc, first, [x.value for x in v])\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")      # (no device even where the machine has one)
    r = subprocess.run([sys.executable, "-c", prog, _lib.LIB_PATH], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n")[0] == "[0, -2, 0] [0, 0, 0, 0] [0, 0, 0, 0]", r.stdout          # -2: GPBC_ERR_NO_DEVICE


def test_small_call_stats_refuse_null(lib):
    """any null out-pointer is GPBC_ERR_INVALID_ARG with a message and nothing written to the others"""
    for hole in range(4):
        v = [ctypes.c_uint64(0xA5A5A5A5A5A5A5A5) for _ in range(4)]
        args = [None if i == hole else ctypes.addressof(x) for i, x in enumerate(v)]
        assert lib.gpbc_small_call_stats(*args) == -1 and b"null" in lib.gpbc_last_error(), hole
        assert all(x.value == 0xA5A5A5A5A5A5A5A5 for x in v), hole
    assert lib.gpbc_small_call_stats(None, None, None, None) == -1


def test_wrapper_rejects_malformed_arguments():
    """ValueError before any C call (no device is touched: this runs without a GPU)"""
    import torch
    from gopairingbasedcryptography_amd import bn254
    z = lambda n: np.zeros(n, dtype=np.uint8)
    t = lambda n: torch.zeros(n, dtype=torch.uint8)
    S = 32
    slots = bn254._slots
    for msm, plain, W in ((bn254.g1_multi_scalar_mul, bn254.g1_sum_segments, 64), (bn254.g2_multi_scalar_mul, bn254.g2_sum_segments, 128)):
        bad = [
            lambda: msm(z(6 * W), z(5 * S), [0, 6]),                                   # one scalar short
            lambda: msm(z(6 * W), z(4 * S), [0, 3, 6]),                                # nk neither n nor n / n_seg
            lambda: msm(z(6 * W), z(3 * S), [0, 2, 6]),                                # shared list, unequal segments
            lambda: msm(z(6 * W), z(7 * S), [0, 6]),                                   # more scalars than points
            lambda: msm(z(6 * W), z(6 * S), [0, 5]),                                   # table does not end at n
            lambda: msm(z(6 * W), z(6 * S), [1, 6]),                                   # does not start at 0
            lambda: msm(z(6 * W), z(6 * S), [0, 4, 3, 6]),                             # not monotone
            lambda: msm(z(6 * W), z(6 * S), [0]),                                      # no segment
            lambda: msm(z(6 * W), z(6 * S), []),
            lambda: msm(z(6 * W + 1), z(6 * S), [0, 6]),                               # not whole points
            lambda: msm(z(6 * W), z(6 * S - 1), [0, 6]),
            lambda: msm(z(6 * W), [1, 2, 3, 4, 5, -1], [0, 6]),                        # negative scalar
            lambda: msm(z(6 * W), [1, 2, 3, 4, 5, 1 << 256], [0, 6]),                  # wider than 256 bits
            lambda: msm(z(6 * W), z(6 * S), [0, 6], out=z(2 * W)),                     # out of the wrong size
            lambda: msm(z(6 * W), z(6 * S), [0, 6], out=np.zeros(W, dtype=np.int8)),
            lambda: msm(z(6 * W), t(6 * S), [0, 6]),                                   # host / device mix
            lambda: msm(z(6 * W), z(6 * S), torch.tensor([0, 6])),
            lambda: msm(t(6 * W), t(6 * S), [0, 6]),                                   # right sizes, but host tensors: not CUDA
            lambda: msm(t(6 * W), t(6 * S), torch.tensor([0, 6], dtype=torch.int32)),  # device table read as uint64
            lambda: msm(t(6 * W).to(torch.int8), t(6 * S), [0, 6]),
            lambda: plain(z(6 * W), [0, 7]),
            lambda: plain(z(6 * W - 1), [0, 6]),
            lambda: plain(t(6 * W), [0, 6]),
        ]
        for i, call in enumerate(bad):
            with pytest.raises(ValueError):
                call()
            assert bn254._slots is slots, i


def test_c_entries_reject_invalid_arguments(lib):
    """GPBC_ERR_INVALID_ARG with a message, nothing written, before any device is touched"""
    p = lambda a: VP(a.ctypes.data)
    seg = lambda *v: np.array(v, dtype=np.uint64)
    wsb = lib.gpbc_multi_scalar_mul_workspace_bytes
    for g2, W in ((0, 64), (1, 128)):
        host = lib.gpbc_g2_multi_scalar_mul if g2 else lib.gpbc_g1_multi_scalar_mul
        dev = lib.gpbc_g2_multi_scalar_mul_dev if g2 else lib.gpbc_g1_multi_scalar_mul_dev
        x, k, out = np.zeros(6 * W, np.uint8), np.zeros(6 * 32 + 3 * W, np.uint8), np.zeros(3 * W, np.uint8)
        ok_seg, uneven, from_one, back = seg(0, 2, 4, 6), seg(0, 1, 4, 6), seg(1, 2, 4, 6), seg(0, 4, 2, 6)       # (kept alive: only addresses cross)
        bad_host = [
            (p(x), p(k), 5, p(ok_seg), 3, p(out)),                       # nk not n and not n / n_seg
            (p(x), p(k), 7, p(ok_seg), 3, p(out)),
            (p(x), p(k), 2, p(uneven), 3, p(out)),                       # shared list of 2, segments of 1 / 3 / 2
            (p(x), None, 6, p(ok_seg), 3, p(out)),                       # scalars missing but counted
            (p(x), p(k), 6, None, 3, p(out)),                            # no table
            (p(x), p(k), 6, p(ok_seg), 0, p(out)),                       # no segment
            (p(x), p(k), 6, p(from_one), 3, p(out)),                     # first entry not 0
            (p(x), p(k), 6, p(back), 3, p(out)),                         # not monotone
            (None, p(k), 6, p(ok_seg), 3, p(out)),                       # NULLs
            (p(x), p(k), 6, p(ok_seg), 3, None),
            (p(x), p(k), 6, p(ok_seg), 3, p(x)),                         # out overlaps the bases
            (p(x), p(k), 6, p(ok_seg), 3, VP(x.ctypes.data + 5 * W)),
            (p(x), None, 0, p(ok_seg), 3, VP(x.ctypes.data + W)),
            (p(x), p(k), 6, p(ok_seg), 3, VP(k.ctypes.data + 5 * 32)),   # out overlaps the scalars
        ]
        for i, a in enumerate(bad_host):
            rc = host(a[0], a[1], a[2], a[3], a[4], a[5])
            assert rc == -1 and lib.gpbc_last_error(), (g2, i)
        ws = np.zeros((1 << 17) + 16, np.uint8)
        ws = ws[-ws.ctypes.data % 16:][:1 << 17]                         # 16-byte aligned
        need = wsb(6, 3, g2)
        assert 0 < need <= ws.size
        bad_dev = [
            (p(x), p(k), 5, p(ok_seg), 6, 3, p(out), p(ws), ws.size),
            (p(x), p(k), 4, p(ok_seg), 6, 3, p(out), p(ws), ws.size),
            (p(x), None, 2, p(ok_seg), 6, 3, p(out), p(ws), ws.size),
            (p(x), p(k), 6, None, 6, 3, p(out), p(ws), ws.size),
            (p(x), p(k), 6, p(ok_seg), 6, 0, p(out), p(ws), ws.size),
            (None, p(k), 6, p(ok_seg), 6, 3, p(out), p(ws), ws.size),
            (p(x), p(k), 6, p(ok_seg), 6, 3, None, p(ws), ws.size),
            (p(x), p(k), 6, p(ok_seg), 6, 3, p(x), p(ws), ws.size),          # overlap
            (p(x), p(k), 6, p(ok_seg), 6, 3, p(out), VP(ws.ctypes.data + 4), ws.size - 4),   # workspace not 16-byte aligned
            (p(x), p(k), 6, p(ok_seg), 6, 3, p(out), p(ws), need - 1),       # workspace one byte short
            (p(x), p(k), 6, p(ok_seg), 6, 3, p(out), None, need),            # no workspace
        ]
        for i, a in enumerate(bad_dev):
            rc = dev(*a, None)
            assert rc == -1 and lib.gpbc_last_error(), (g2, i)
        assert b"workspace" in lib.gpbc_last_error()
        assert not out.any() and not x.any() and not ws.any() and not k.any()


def test_workspace_is_bounded_independently_of_the_segment_length(lib):
    """lane blocks for at most 131072 pieces, piece values for at most 131072 + n_seg pieces and their folds: the same bound for a
    64-term segment as for a 2^30-term one"""
    wsb = lib.gpbc_multi_scalar_mul_workspace_bytes
    for g2, W in ((False, 64), (True, 128)):
        G = gc.group(g2)
        block = 4 * (G * (1024 if g2 else 512) + 128 + (64 if g2 else 32))   # G tables, the window words and the accumulator of one lane
        assert wsb(1 << 26, 1, g2) == wsb(1 << 30, 1, g2) <= gc.FILL * block + W * (gc.FILL + gc.FILL // 8) + 3 * 256
        for n_seg in (1, 4, 4096, 1 << 16, 1 << 20):
            for m in (1, 4, 16, 64, 4096):
                P = n_seg * gc.pieces(n_seg * m, n_seg, True, g2)
                assert P <= gc.FILL + n_seg
                assert 0 < wsb(n_seg * m, n_seg, g2) <= min(P, gc.FILL) * block + W * (P + P // 8) + 3 * 256, (n_seg, m)      # the header's bound
        assert wsb(0, 1, g2) == block + (-block % 256) and wsb(5, 0, g2) == 0     # an empty segment is still one piece (it writes one); no segment, nothing


def test_no_cpu_fallback_for_multi_scalar_mul(lib):
    """without a GPU a well-formed call returns a negative status, writes nothing and leaves a message"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gopairingbasedcryptography_amd import bn254, EngineError
    for g2 in GROUPS:
        W = gc.BYTES[g2]
        x, out = np.ascontiguousarray(gc.take(gc.pool(g2)["pt"], 4)).reshape(-1), np.zeros((2, W), np.uint8)
        msm, plain = (bn254.g2_multi_scalar_mul, bn254.g2_sum_segments) if g2 else (bn254.g1_multi_scalar_mul, bn254.g1_sum_segments)
        with pytest.raises(EngineError):
            msm(x, [1, 2, 3, 4], [0, 2, 4], out=out)
        with pytest.raises(EngineError):
            plain(x, [0, 4])
        seg = np.array([0, 2, 4], dtype=np.uint64)
        host = lib.gpbc_g2_multi_scalar_mul if g2 else lib.gpbc_g1_multi_scalar_mul
        assert host(x.ctypes.data, None, 0, seg.ctypes.data, 2, out.ctypes.data) < 0 and lib.gpbc_last_error()
        assert not out.any()
