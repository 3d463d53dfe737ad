"""Segmented inner products in Fr and GT.Equal on the MI355X (run with -m gpu): k_fr_dot_segments through bn254.fr_dot_segments /
fr_sum_segments and the C entries, k_gt_equal through bn254.gt_equal.  Everything is bit-exact against Python integers (tests/fr_dot_cases.py)
or byte comparisons:

  * segment lengths 0, 1, 2, 3, 63, 64, 65 and 129 in one call; wavefronts with G and G + 1 rounds side by side; a piece that passes a
    reduction; cut segments of exactly two and of three levels; all three modes (a b per element, a shared list, the plain sum);
  * every value r - 1, every value 2^256 - 1 (acting as its residue), zeros;
  * the host form and the _dev form give equal bytes (table on the host and on the device); out 16-byte aligned and not, a caller's
    workspace with a guard behind it;
  * a _dev table with offsets beyond n is clamped: the sums are those of the clamped table (the kernel clamps before it forms an address);
  * gt_equal: rows that differ only in byte 0 or only in byte 383, equal rows, one b for all, n = 1, 64, 65 and 300, rows that are
    only 4-byte aligned."""
import ctypes

import numpy as np
import pytest

import fr_dot_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_want = {}


def want(name, mode):
    """the expectation of a case, computed once"""
    if (name, mode) not in _want:
        a, b, seg, shared = fc.case_inputs(name, mode)
        _want[name, mode] = fc.expect(a, b, seg, shared=shared)
    return _want[name, mode]


@pytest.mark.parametrize("name", list(fc.CASES))
def test_cases_host_and_device(eng, name):
    import torch
    for mode in fc.case_modes(fc.CASES[name][0]):
        a, b, seg, _ = fc.case_inputs(name, mode)
        w = want(name, mode)
        da, db = to_dev(a), None if b is None else to_dev(b)
        dev = eng.fr_dot_segments(da, db, seg)
        assert dev.is_cuda and dev.shape == w.shape and (dev.cpu().numpy() == w).all(), (name, mode, "device, table on the host")
        dev2 = eng.fr_dot_segments(da, db, to_dev(seg.astype(np.int64)))
        assert bool((dev2 == dev).all()), (name, mode, "device, table on the device")
        if name != "three_levels" or mode == "dot":
            host = eng.fr_dot_segments(a, b, seg)
            assert isinstance(host, np.ndarray) and host.tobytes() == w.tobytes(), (name, mode, "host")
    torch.cuda.synchronize()


def test_sum_segments_and_python_integers(eng):
    a, _, seg, _ = fc.case_inputs("short", "sum")
    assert eng.fr_sum_segments(a, seg).tobytes() == want("short", "sum").tobytes()
    assert fc.ints(eng.fr_dot_segments([1, 2, 3, fc.R - 1], [5, 6, 7, 2**256 - 1], [0, 2, 2, 4])) == [17, 0, (21 + (fc.R - 1) * (2**256 - 1)) % fc.R]
    assert fc.ints(eng.fr_dot_segments(to_dev(fc.rows_of([1, 2, 3, 4])), [10, 100], [0, 2, 4]).cpu().numpy()) == [210, 430]      # a host list beside device rows


@pytest.mark.parametrize("value", sorted(fc.EXTREMES))
def test_extreme_values(eng, value):
    a, b, seg = fc.extreme_inputs(fc.EXTREMES[value])
    for bb in (b, None):
        w = fc.expect(a, bb, seg)
        got = eng.fr_dot_segments(to_dev(a), None if bb is None else to_dev(bb), seg).cpu().numpy()
        assert (got == w).all() and all(v < fc.R for v in fc.ints(got))
    # ... and through the cut: one segment of the same elements
    one = [0, len(a)]
    assert fc.pieces(len(a), 1, True) > 1
    assert (eng.fr_dot_segments(to_dev(a), to_dev(b), one).cpu().numpy() == fc.expect(a, b, one)).all()


def test_dev_table_beyond_n_is_clamped(eng):
    """the C entry on a table whose offsets pass n: every offset is clamped to n before an address is formed"""
    import torch
    lib = eng._lib.load()
    n = 200
    a, b = fc.rand_rows("clamp/a", n), fc.rand_rows("clamp/b", n)
    seg = np.array([0, 70, 150, 260, 1 << 40, (1 << 63) + 5], dtype=np.uint64)
    w = fc.expect(a, b, seg, n=n)
    assert fc.ints(w)[3:] == [0, 0] and fc.ints(w)[2] == fc.ints(fc.expect(a, b, [0, 150, 200]))[1]
    da, db, dseg = to_dev(a), to_dev(b), to_dev(seg.view(np.int64))
    out = torch.full((5 * 32 + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert lib.gpbc_fr_dot_segments_dev(da.data_ptr(), db.data_ptr(), n, dseg.data_ptr(), n, 5, out.data_ptr(), None, 0, st) == 0
    torch.cuda.synchronize()
    assert (out[:160].cpu().numpy().reshape(5, 32) == w).all() and bool((out[160:] == 0xA5).all())
    # a shared list ends a segment after nb elements
    shared = np.array([0, 100, 200], dtype=np.uint64)
    long_first = np.array([0, 150, 200], dtype=np.uint64)
    assert lib.gpbc_fr_dot_segments_dev(da.data_ptr(), db.data_ptr(), 100, to_dev(long_first.view(np.int64)).data_ptr(), n, 2, out.data_ptr(), None, 0, st) == 0
    torch.cuda.synchronize()
    assert (out[:64].cpu().numpy().reshape(2, 32) == fc.expect(a, b[:100], long_first, n=n, shared=True)).all()
    assert (eng.fr_dot_segments(da, db[:100].contiguous(), shared).cpu().numpy() == fc.expect(a, b[:100], shared, shared=True)).all()


def test_caller_buffers_alignment_and_workspace(eng):
    import torch
    a, b, seg, _ = fc.case_inputs("cut_uneven", "dot")
    w = want("cut_uneven", "dot")
    n, n_seg = len(a), len(seg) - 1
    wsb = eng._lib.load().gpbc_fr_dot_segments_workspace_bytes(n, n_seg)
    assert wsb > 0
    da, db = to_dev(a), to_dev(b)
    for shift in (0, 4, 8):                                                                # out 16-byte aligned and not
        ws = torch.zeros(wsb + 512, dtype=torch.uint8, device="cuda")
        buf = torch.full((n_seg * 32 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        out = eng.fr_dot_segments(da, db, seg, out=buf[shift:shift + n_seg * 32], workspace=ws[:wsb])
        assert (out.cpu().numpy().reshape(n_seg, 32) == w).all(), shift
        assert bool((buf[:shift] == 0x5A).all()) and bool((buf[shift + n_seg * 32:] == 0x5A).all()) and bool((ws[wsb:] == 0).all())
    # inputs that are only 4-byte aligned take the dword loads
    raw = torch.zeros(n * 32 + 16, dtype=torch.uint8, device="cuda")
    raw[4:4 + n * 32] = da.reshape(-1)
    assert (eng.fr_dot_segments(raw[4:4 + n * 32], db, seg).cpu().numpy() == w).all()
    h = np.zeros((n_seg, 32), dtype=np.uint8)
    assert eng.fr_dot_segments(a, b, seg, out=h) is h and (h == w).all()
    from gopairingbasedcryptography_amd import EngineError
    with pytest.raises(EngineError):
        eng.fr_dot_segments(da, db, seg, out=da.reshape(-1)[:n_seg * 32])                   # out overlaps a: refused by the C entry
    with pytest.raises(ValueError):
        eng.fr_dot_segments(da, db, seg, workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        eng.fr_dot_segments(da, db, to_dev(np.array([0, 5, 3, n], dtype=np.int64)))         # a device table is validated on the device
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_gt_equal(eng, n):
    import torch
    rng = np.random.default_rng(fc.hash_tag("gt_equal/%d" % n))
    a = rng.integers(0, 256, size=(n, 384), dtype=np.uint8)
    b = a.copy()
    kinds = np.arange(n) % 4                                                               # equal, byte 0, byte 383, both
    b[kinds == 1, 0] ^= 1
    b[kinds == 2, 383] ^= 0x80
    b[kinds == 3, 0] ^= 0x10
    b[kinds == 3, 383] ^= 1
    w = (kinds == 0).astype(np.uint8)
    got = eng.gt_equal(to_dev(a), to_dev(b))
    assert got.is_cuda and got.dtype == torch.uint8 and (got.cpu().numpy() == w).all()
    assert (eng.gt_equal(a, b) == w).all()
    assert bool((eng.gt_equal(to_dev(a), to_dev(a)) == 1).all())
    # one b for all: row j of a is the b
    j = n // 2
    a2 = a.copy()
    a2[::3] = a[j]
    w1 = (a2 == a[j]).all(1).astype(np.uint8)
    assert w1.sum() >= 1 and (eng.gt_equal(to_dev(a2), to_dev(a[j:j + 1])).cpu().numpy() == w1).all()
    assert (eng.gt_equal(a2, a[j]) == w1).all()
    # rows that are only 4-byte aligned
    raw = torch.zeros(n * 384 + 16, dtype=torch.uint8, device="cuda")
    raw[4:4 + n * 384] = to_dev(a).reshape(-1)
    out = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    eng.gt_equal(raw[4:4 + n * 384], to_dev(b), out=out[:n])
    assert (out[:n].cpu().numpy() == w).all() and bool((out[n:] == 0xA5).all())
