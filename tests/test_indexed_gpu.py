"""The indexed sums over fixed-base tables on the device (run with -m gpu): gpbc_fixed_base_indexed, host and _dev forms, numpy and CUDA
tensors on a stream of their own, G1 and G2, on the corpus of tests/indexed_cases.py against the oracle's scalar multiplication and sum
over the selected bases, bit for bit.  A table of 6 bases (one the point at infinity, two equal), 323 outputs (not a multiple of 64,
more than one workgroup), 1 / 2 / 3 / 16 terms, 1 / 19 / 323 index rows (19: the period wraps and does not divide n)."""
import ctypes

import numpy as np
import pytest

import indexed_cases as ic

pytestmark = pytest.mark.gpu
N = 323


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


@pytest.fixture(scope="module", params=[False, True], ids=["g1", "g2"])
def table(eng, oracle, request):
    t = eng.FixedBase(ic.bases(oracle, request.param), g2=request.param)
    yield t
    t.close()


def run(table, case, tensors):
    k = ic.rows([v for r in case["scalars"] for v in r])
    if not tensors:
        out, ok = table.indexed(case["index"], k, terms=case["terms"])
        assert isinstance(out, np.ndarray) and isinstance(ok, np.ndarray)
        return out, ok
    import torch
    side = torch.cuda.Stream()
    idx, kd = torch.from_numpy(case["index"].view(np.int32).copy()).cuda(), torch.from_numpy(k).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out, ok = table.indexed(idx, kd, terms=case["terms"])
    side.synchronize()
    assert out.is_cuda and ok.is_cuda
    return out.cpu().numpy(), ok.cpu().numpy()


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("P", [1, 19, N])
@pytest.mark.parametrize("terms", [1, 2, 3, 16])
def test_corpus_against_the_oracle(table, oracle, terms, P, tensors):
    case = ic.indexed_case(N, terms, P)
    want, want_ok = ic.expected(oracle, table.g2, case, key=(N, terms, P))
    out, ok = run(table, case, tensors)
    assert out.shape == (N, table.width) and ok.tolist() == want_ok.tolist()
    bad = [i for i in range(N) if out[i].tobytes() != want[i].tobytes()]
    assert not bad, (bad[:8], case["planted"])
    if P >= 16:                                                                        # index nbase and 0xfffffffe: zero rows, ok = 0, neighbours intact (above)
        assert (want_ok == 0).sum() >= 2 and not out[want_ok == 0].any()


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_invalid_index_without_ok_out(eng, table, oracle, tensors):
    """ok_out NULL: the same outputs, the invalid rows all zero, every neighbour intact"""
    import torch
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    case = ic.indexed_case(N, 2, N)
    want, want_ok = ic.expected(oracle, table.g2, case, key=(N, 2, N))
    k = ic.rows([v for r in case["scalars"] for v in r])
    idx = np.ascontiguousarray(case["index"])
    if tensors:
        kd, idd = torch.from_numpy(k).cuda(), torch.from_numpy(idx.view(np.int32).copy()).cuda()
        out = torch.full((N + 1, table.width), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _lib.check(lib.gpbc_fixed_base_indexed_dev(table._h, idd.data_ptr(), N, 2, kd.data_ptr(), N, out.data_ptr(), None, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        out = out.cpu().numpy()
    else:
        out = np.full((N + 1, table.width), 0xA5, dtype=np.uint8)
        _lib.check(lib.gpbc_fixed_base_indexed(table._h, idx.ctypes.data, N, 2, k.ctypes.data, N, out.ctypes.data, None))
    assert (want_ok == 0).sum() >= 2 and out[:N].tobytes() == want.tobytes() and (out[N] == 0xA5).all()


def test_one_base_table_is_mul_and_dense_row_is_msm(eng, oracle):
    ks = [0, 1, ic.R - 1, ic.R, ic.R + 1, ic.TOP] + [ic.o.bench_scalar("indexed-mul", i) for i in range(61)]
    for g2 in (False, True):
        b = ic.bases(oracle, g2)
        one = eng.FixedBase(b[:1], g2=g2)
        out, ok = one.indexed([[0]], ic.rows(ks), terms=1)
        assert out.tobytes() == np.asarray(one.mul(ic.rows(ks))).tobytes() and ok.all()
        one.close()
        full = eng.FixedBase(b, g2=g2)
        k = ic.rows([ic.o.bench_scalar("indexed-msm", i) for i in range(5 * ic.NBASE)])
        out, ok = full.indexed([list(range(ic.NBASE))], k, terms=ic.NBASE)
        assert out.tobytes() == np.asarray(full.msm(k)).tobytes() and ok.all() and out.shape == (5, 128 if g2 else 64)
        full.close()


def test_entry_refuses_bad_sizes_overlap_and_out_argument(eng, table):
    import torch
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    VP, SZ = ctypes.c_void_p, ctypes.c_size_t
    buf = np.zeros(64 * 128, np.uint8)
    p = VP(buf.ctypes.data)
    for terms, rows, n, what in ((0, 1, 4, b"terms"), (17, 1, 4, b"terms"), (1, 0, 4, b"n_index_rows"), (1, 5, 4, b"n_index_rows")):
        assert lib.gpbc_fixed_base_indexed(table._h, p, SZ(rows), SZ(terms), p, SZ(n), VP(buf.ctypes.data + 4096), None) == -1 and what in lib.gpbc_last_error()
    assert lib.gpbc_fixed_base_indexed(table._h, None, SZ(1), SZ(1), p, SZ(4), VP(buf.ctypes.data + 4096), None) == -1 and b"null" in lib.gpbc_last_error()
    assert lib.gpbc_fixed_base_indexed(table._h, p, SZ(1), SZ(1), VP(buf.ctypes.data + 64), SZ(4), VP(buf.ctypes.data + 128), None) == -1 and b"overlaps" in lib.gpbc_last_error()
    assert lib.gpbc_fixed_base_indexed(table._h, p, SZ(1), SZ(1), p, SZ(0), p, None) == 0 and not buf.any()
    out = torch.zeros((4, table.width), dtype=torch.uint8, device="cuda")
    k = torch.from_numpy(ic.rows([1, 2, 3, 4])).cuda()
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    got, ok = table.indexed(idx, k, terms=1, out=out)
    assert got is out and ok.cpu().numpy().all()
    with pytest.raises(ValueError):
        table.indexed(np.zeros(1, np.uint32), k, terms=1)                              # host index, device scalars
