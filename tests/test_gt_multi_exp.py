"""Segmented GT multi-exponentiation (csrc/gtmexp29.hip.hpp, csrc/gpbc_gtmexp.hip), CPU part.

hc_gt_multi_exp_pair (tools/bounds_check.cpp) runs the plan and the lane functions of gpbc_gt_multi_exp_dev on the host with
-DGPBC_BOUNDS — the same piece cut, the same f12p_multi_exp / f12p_product per lane pair, the same folds — against the oracle's
gt_exp folded with gt_mul, bit for bit, on the case lists of gt_multi_exp_cases.py.  The loop multiplies into the accumulator up
to four times in a row with no squaring between, and folds products of products: in that build every product asserts its int64
columns and every table row its limb range, so a run that finishes is the overflow proof.  Then the wrapper's and the C entries'
argument checks, which need no device."""
import ctypes

import numpy as np
import pytest

from bounds_harness import hc  # noqa: F401  (the fixture)
import gt_multi_exp_cases as gc

VP, SZ = ctypes.c_void_p, ctypes.c_size_t


def hc_run(hc, x, k, seg):
    x = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, gc.GT)
    kr = gc.krows(k) if k is not None and len(k) else np.zeros((1, 32), dtype=np.uint8)
    s = np.array(seg, dtype=np.uint64)
    out = np.full((len(seg) - 1, gc.GT), 0xA5, dtype=np.uint8)
    hc.hc_gt_multi_exp_pair(x.ctypes.data if len(x) else None, kr.ctypes.data if k is not None else None, len(k) if k is not None else 0,
                            s.ctypes.data, len(x), len(seg) - 1, out.ctypes.data)
    return out


def test_plan_restated():
    """the cut the case lists aim at: J from the sizes alone, and the boundaries named in gt_multi_exp_cases"""
    assert [gc.pieces(L, 1, True) for L in (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65)] == [1, 1, 1, 2, 2, 3, 4, 4, 15, 16, 16]
    assert [gc.pieces(L, 1, False) for L in (15, 16, 17, 127, 128, 129)] == [1, 2, 2, 15, 16, 16]
    assert gc.pieces(1 << 20, 1, False) == 65536 and gc.pieces(1 << 20, 16, True) == 4096 and gc.pieces(1 << 20, 1 << 16, True) == 1
    assert gc.pieces(1 << 18, 1 << 12, True) == 16 and gc.pieces(192, 11, True) == 4


def test_cases_under_bounds(hc, oracle):
    """every case of the list against oracle gt_exp folded with gt_mul, bit for bit; a finished run is the overflow proof"""
    seen = set()
    for label, x, k, seg, shared in gc.cases(oracle):
        got = hc_run(hc, x, k, seg)
        want = gc.expect(oracle, x, k, seg, shared)
        assert (got == want).all(), (label, np.nonzero((got != want).any(axis=1))[0][:8])
        seen.add(label)
    assert len(seen) > 40


def test_table_past_n_is_clamped_as_on_the_device(hc, oracle):
    """what a device-resident table can do: the last offset lies past n.  The harness runs the kernels' own segment range, which clamps
    every offset to n: 6 factors, table [0, 4, 9] -> out[1] is the product over x[4:6], and nothing past x[5] is read (x and k hold
    exactly 6 rows)"""
    x, k = gc.take(gc.pool(oracle)["pair"], 6), gc.rand_exps("past-n", 6)
    got = hc_run(hc, x, k, [0, 4, 9])
    assert (got == gc.expect(oracle, x, k, [0, 4, 6], False)).all()


def test_one_element_segments_are_gt_exp(hc, oracle):
    """segments of one element are GT.Exp itself, for the harness form of k_gt_exp too (hc_gt_exp_pair)"""
    p = gc.pool(oracle)
    x = np.concatenate([p["pair"][:4], p["miller"][:1]])
    k = gc.rand_exps("single", 5)
    got = hc_run(hc, x, k, list(range(6)))
    ref = np.zeros_like(got)
    hc.hc_gt_exp_pair(VP(np.ascontiguousarray(x).ctypes.data), VP(gc.krows(k).ctypes.data), SZ(5), VP(ref.ctypes.data))
    assert (got == ref).all() and (got == oracle.gt_exp(x, gc.krows(k))).all()


def test_bound_margins_after_multi_exp(hc, oracle):
    p = gc.pool(oracle)
    hc_run(hc, gc.take(p["pair"], 9), gc.rand_exps("bm", 9), [0, 9])
    st = np.zeros(7)
    hc.hc_stats(st.ctypes.data_as(VP))
    assert 0 < st[0] < 2.0**63 and st[1] < 2.0**31


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
    G, S = gc.GT, 32
    bad = [
        lambda: bn254.gt_multi_exp(z(6 * G), z(5 * S), [0, 6]),                           # one exponent short
        lambda: bn254.gt_multi_exp(z(6 * G), z(4 * S), [0, 3, 6]),                        # nk neither n nor n / n_seg
        lambda: bn254.gt_multi_exp(z(6 * G), z(3 * S), [0, 2, 6]),                        # shared list, unequal segments
        lambda: bn254.gt_multi_exp(z(6 * G), z(7 * S), [0, 6]),                           # more exponents than elements
        lambda: bn254.gt_multi_exp(z(6 * G), z(6 * S), [0, 5]),                           # table does not end at n
        lambda: bn254.gt_multi_exp(z(6 * G), z(6 * S), [1, 6]),                           # does not start at 0
        lambda: bn254.gt_multi_exp(z(6 * G), z(6 * S), [0, 4, 3, 6]),                     # not monotone
        lambda: bn254.gt_multi_exp(z(6 * G), z(6 * S), [0]),                              # no segment
        lambda: bn254.gt_multi_exp(z(6 * G), z(6 * S), []),
        lambda: bn254.gt_multi_exp(z(6 * G + 1), z(6 * S), [0, 6]),                       # not whole elements
        lambda: bn254.gt_multi_exp(z(6 * G), z(6 * S - 1), [0, 6]),
        lambda: bn254.gt_multi_exp(z(6 * G), [1, 2, 3, 4, 5, -1], [0, 6]),                # negative exponent
        lambda: bn254.gt_multi_exp(z(6 * G), [1, 2, 3, 4, 5, 1 << 256], [0, 6]),          # wider than 256 bits
        lambda: bn254.gt_multi_exp(z(6 * G), z(6 * S), [0, 6], out=z(2 * G)),             # out of the wrong size
        lambda: bn254.gt_multi_exp(z(6 * G), z(6 * S), [0, 6], out=np.zeros(G, dtype=np.int8)),
        lambda: bn254.gt_multi_exp(z(6 * G), t(6 * S), [0, 6]),                           # host / device mix
        lambda: bn254.gt_multi_exp(z(6 * G), z(6 * S), torch.tensor([0, 6])),
        lambda: bn254.gt_multi_exp(t(6 * G), t(6 * S), [0, 6]),                           # right sizes, but host tensors: not CUDA
        lambda: bn254.gt_multi_exp(t(6 * G), t(6 * S), torch.tensor([0, 6], dtype=torch.int32)),   # device table read as uint64
        lambda: bn254.gt_multi_exp(t(6 * G).to(torch.int8), t(6 * S), [0, 6]),
        lambda: bn254.gt_prod(z(6 * G), [0, 7]),
        lambda: bn254.gt_prod(z(6 * G - 1)),
        lambda: bn254.gt_prod(t(6 * G)),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()


def test_c_entries_reject_invalid_arguments(lib):
    """GPBC_ERR_INVALID_ARG with a message, nothing written, before any device is touched"""
    G = gc.GT
    x, k, out = np.zeros(6 * G, np.uint8), np.zeros(6 * 32, np.uint8), np.zeros(3 * G, np.uint8)
    p = lambda a: VP(a.ctypes.data)
    seg = lambda *v: np.array(v, dtype=np.uint64)
    host, dev, wsb = lib.gpbc_gt_multi_exp, lib.gpbc_gt_multi_exp_dev, lib.gpbc_gt_multi_exp_workspace_bytes
    ok_seg, uneven, from_one, back = seg(0, 2, 4, 6), seg(0, 1, 4, 6), seg(1, 2, 4, 6), seg(0, 4, 2, 6)       # (kept alive: only addresses cross)
    bad_host = [
        (p(x), p(k), 5, p(ok_seg), 3, p(out)),                       # nk not n and not n / n_seg
        (p(x), p(k), 7, p(ok_seg), 3, p(out)),
        (p(x), p(k), 2, p(uneven), 3, p(out)),              # shared list of 2, segments of 1 / 3 / 2
        (p(x), None, 6, p(ok_seg), 3, p(out)),                       # exponents missing but counted
        (p(x), p(k), 6, None, 3, p(out)),                            # no table
        (p(x), p(k), 6, p(ok_seg), 0, p(out)),                       # no segment
        (p(x), p(k), 6, p(from_one), 3, p(out)),              # first entry not 0
        (p(x), p(k), 6, p(back), 3, p(out)),              # not monotone
        (None, p(k), 6, p(ok_seg), 3, p(out)),                       # NULLs
        (p(x), p(k), 6, p(ok_seg), 3, None),
        (p(x), p(k), 6, p(ok_seg), 3, p(x)),                         # out overlaps x
        (p(x), p(k), 6, p(ok_seg), 3, VP(x.ctypes.data + 5 * G)),
        (p(x), None, 0, p(ok_seg), 3, VP(x.ctypes.data + G)),
        (p(x), p(k), 6, p(ok_seg), 3, p(k)),                         # out overlaps k
        (p(x), p(k), 2, p(ok_seg), 3, VP(k.ctypes.data + 32)),       # out overlaps a shared list of 2
    ]
    for i, a in enumerate(bad_host):
        rc = host(a[0], a[1], SZ(a[2]), a[3], SZ(a[4]), a[5])
        assert rc == -1 and lib.gpbc_last_error(), i
    ws = np.zeros(1 << 16, np.uint8)
    need = wsb(6, 3)
    assert 0 < need <= 6 * 32768 + 4096
    bad_dev = [
        (p(x), p(k), 5, p(ok_seg), 6, 3, p(out), p(ws), ws.size),
        (p(x), p(k), 4, p(ok_seg), 6, 3, p(out), p(ws), ws.size),
        (p(x), None, 2, p(ok_seg), 6, 3, p(out), p(ws), ws.size),
        (p(x), p(k), 6, None, 6, 3, p(out), p(ws), ws.size),
        (p(x), p(k), 6, p(ok_seg), 6, 0, p(out), p(ws), ws.size),
        (None, p(k), 6, p(ok_seg), 6, 3, p(out), p(ws), ws.size),
        (p(x), p(k), 6, p(ok_seg), 6, 3, None, p(ws), ws.size),
        (p(x), p(k), 6, p(ok_seg), 6, 3, p(x), p(ws), ws.size),          # overlap
        (p(x), p(k), 6, p(ok_seg), 6, 3, p(k), p(ws), ws.size),          # out overlaps k
        (p(x), p(k), 6, p(ok_seg), 6, 3, p(out), p(ws), need - 1),       # workspace one byte short
        (p(x), p(k), 6, p(ok_seg), 6, 3, p(out), None, need),            # no workspace
    ]
    for i, a in enumerate(bad_dev):
        rc = dev(a[0], a[1], SZ(a[2]), a[3], SZ(a[4]), SZ(a[5]), a[6], a[7], SZ(a[8]), None)
        assert rc == -1 and lib.gpbc_last_error(), i
    assert b"workspace" in lib.gpbc_last_error()
    assert not out.any() and not x.any() and not k.any() and not ws.any()


def test_workspace_is_bounded_independently_of_the_segment_length(lib):
    """tables for at most 65536 pieces of 32 KiB, piece values for at most 65536 + n_seg pieces and their folds: the same bound for
    a 64-factor segment as for a 2^20-factor one"""
    wsb = lib.gpbc_gt_multi_exp_workspace_bytes
    cap = 65536 * 32768 + 432 * (65536 + 1) + 3 * 256
    assert wsb(64, 1) <= 16 * 32768 + 16 * 432 + 3 * 256
    assert wsb(1 << 20, 1) <= cap and wsb(1 << 26, 1) <= cap and wsb(1 << 26, 1) == wsb(1 << 30, 1)
    for n_seg in (1, 4, 4096, 1 << 16, 1 << 20):
        for m in (1, 4, 16, 64, 4096):
            P = n_seg * gc.pieces(n_seg * m, n_seg, True)
            assert P <= 65536 + n_seg
            assert wsb(n_seg * m, n_seg) <= min(P, 65536) * 32768 + 432 * P + 3 * 256
    assert wsb(0, 1) == 32768 and wsb(5, 0) == 0                  # an empty segment is still one piece (it writes one); no segment, nothing


def test_no_cpu_fallback_for_gt_multi_exp(lib):
    """without a GPU a well-formed call returns a negative status, writes nothing and leaves a message"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gopairingbasedcryptography_amd import bn254, EngineError
    x, out = np.zeros(4 * gc.GT, np.uint8), np.zeros((2, gc.GT), np.uint8)
    with pytest.raises(EngineError):
        bn254.gt_multi_exp(x, [1, 2, 3, 4], [0, 2, 4], out=out)
    with pytest.raises(EngineError):
        bn254.gt_prod(x)
    seg = np.array([0, 2, 4], dtype=np.uint64)
    assert lib.gpbc_gt_multi_exp(VP(x.ctypes.data), None, SZ(0), VP(seg.ctypes.data), SZ(2), VP(out.ctypes.data)) < 0 and lib.gpbc_last_error()
    assert not out.any()
