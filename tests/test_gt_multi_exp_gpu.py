"""Segmented GT multi-exponentiation on the MI355X (run with -m gpu): k_gt_multi_exp / k_gt_prod through the host-pointer and the
device entries.

  * the case lists of tests/gt_multi_exp_cases.py against the oracle (gt_exp folded with gt_mul), bit for bit: host arrays, CUDA
    tensors with the table on the host and on the device, and once more in a process bound to the device list {0, 0} with calls
    large enough to cross the shard split (whole segments per shard);
  * agreement of forms, bit for bit (canonical outputs leave no tolerance): one-element segments == gt_exp; gt_prod == a left fold
    of gt_mul; 2^16 segments x 16 factors and 4 segments x 2^16 factors against the engine's own gt_exp + folded gt_mul, with
    oracle checks at the first, the last and the boundary positions; more pieces than one launch takes (65536);
  * wrong inputs are refused on the host before anything is launched on them."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import gt_multi_exp_cases as gc

pytestmark = pytest.mark.gpu
GT = gc.GT


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fold_mul(eng, e, n_seg, m):
    """prod over the m columns of e [n_seg * m, 384] with the engine's elementwise gt_mul: log2(m) rounds (m a power of two)"""
    cur = e.reshape(n_seg, m, GT)
    while m > 1:
        cur = eng.gt_mul(cur[:, 0::2].contiguous().reshape(-1), cur[:, 1::2].contiguous().reshape(-1)).reshape(n_seg, m // 2, GT)
        m //= 2
    return cur.reshape(n_seg, GT)


def test_cases_host_and_device(eng, oracle):
    import torch
    assert gc.run_engine_cases(eng, oracle) == []
    assert gc.run_engine_cases(eng, oracle, put=to_dev) == []
    assert gc.run_engine_cases(eng, oracle, put=to_dev, table_on_device=True) == []
    torch.cuda.synchronize()


def test_host_entry_across_the_shard_split():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gt_multi_exp_cases.py"), "0", "0"], capture_output=True, text=True, timeout=900)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "devices 2 failures []" in r.stdout


def test_one_element_segments_are_gt_exp(eng, oracle):
    import torch
    p = gc.pool(oracle)
    n = 5000
    rows = np.concatenate([p["pair"], p["miller"]])
    x = to_dev(rows[np.arange(n) % len(rows)])
    k = to_dev(gc.krows(gc.EDGE_EXPS + gc.rand_exps("single", n - len(gc.EDGE_EXPS))))
    got = eng.gt_multi_exp(x.reshape(-1), k.reshape(-1), to_dev(np.arange(n + 1, dtype=np.int64)))
    assert bool((got == eng.gt_exp(x.reshape(-1), k.reshape(-1))).all())
    h = eng.gt_multi_exp(x[:40].cpu().numpy().reshape(-1), k[:40].cpu().numpy().reshape(-1), list(range(41)))
    assert (h == got[:40].cpu().numpy()).all() and (h == oracle.gt_exp(x[:40].cpu().numpy(), k[:40].cpu().numpy())).all()
    torch.cuda.synchronize()


def test_gt_prod_is_a_left_fold_of_gt_mul(eng, oracle):
    p = gc.pool(oracle)
    n = 300
    rows = np.concatenate([p["pair"], p["miller"], p["inv"][:5]])
    x = np.ascontiguousarray(rows[(np.arange(n) * 7) % len(rows)])
    acc = p["one"][0]
    for i in range(n):
        acc = eng.gt_mul(acc, x[i])[0]
    assert (eng.gt_prod(x.reshape(-1)) == acc).all() and eng.gt_prod(x.reshape(-1)).shape == (GT,)
    assert (eng.gt_prod(to_dev(x.reshape(-1))).cpu().numpy() == acc).all()
    assert (eng.gt_prod(x.reshape(-1), [0, 100, 100, n])[1] == p["one"][0]).all()


def sized_inputs(eng, n, tag):
    """n pairing values e(g1, g2)^a_i made with gt_exp, and n random 256-bit exponents, device-resident"""
    g1, g2 = eng.generators()
    e = eng.pair_batch(g1, g2)
    rng = np.random.default_rng(gc.hash_tag(tag))
    a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 31] &= 0x1F
    x = eng.gt_exp(to_dev(np.tile(e.reshape(1, GT), (n, 1))).reshape(-1), to_dev(a).reshape(-1))
    k = to_dev(rng.integers(0, 256, size=(n, 32), dtype=np.uint8))
    return x, k


def test_2_16_segments_of_16(eng, oracle):
    import torch
    n_seg, m = 1 << 16, 16
    x, k = sized_inputs(eng, n_seg * m, "many-short")
    table = np.arange(0, n_seg * m + 1, m, dtype=np.uint64)
    got = eng.gt_multi_exp(x.reshape(-1), k.reshape(-1), table)
    want = fold_mul(eng, eng.gt_exp(x.reshape(-1), k.reshape(-1)), n_seg, m)
    wrong = torch.nonzero((got != want).any(dim=1)).flatten()
    print("2^16 x 16: %d of %d segments differ from gt_exp + gt_mul" % (wrong.numel(), n_seg))
    assert wrong.numel() == 0, wrong[:8].tolist()
    got2 = eng.gt_multi_exp(x.reshape(-1), k.reshape(-1), to_dev(table.astype(np.int64)))          # the table on the device
    assert bool((got2 == got).all())
    for s in (0, 1, 31, 32, 32767, 32768, n_seg - 2, n_seg - 1):                                  # first, last, wavefront and half-chip positions
        xs, ks = x.reshape(-1, GT)[s * m:(s + 1) * m].cpu().numpy(), k.reshape(-1, 32)[s * m:(s + 1) * m].cpu().numpy()
        w = gc.expect_threads(oracle, xs, [int.from_bytes(r.tobytes(), "little") for r in ks], [0, m], False)
        assert (got[s].cpu().numpy() == w[0]).all(), s
    # one exponent list for all segments
    ks = gc.rand_exps("shared-16", m)
    got3 = eng.gt_multi_exp(x.reshape(-1), ks, table)
    kt = to_dev(np.tile(gc.krows(ks), (n_seg, 1)))
    assert bool((got3 == fold_mul(eng, eng.gt_exp(x.reshape(-1), kt.reshape(-1)), n_seg, m)).all())


def test_4_segments_of_2_16(eng, oracle):
    import torch
    n_seg, m = 4, 1 << 16
    x, k = sized_inputs(eng, n_seg * m, "few-long")
    table = [0, m, 2 * m, 3 * m, 4 * m]
    got = eng.gt_multi_exp(x.reshape(-1), k.reshape(-1), table)
    want = fold_mul(eng, eng.gt_exp(x.reshape(-1), k.reshape(-1)), n_seg, m)
    assert bool((got == want).all())
    assert gc.pieces(n_seg * m, n_seg, True) == 16384                 # 65536 pieces of 4 factors, then four product folds
    # every segment holds piece boundaries at every fold level: all four against the oracle
    kint = [int.from_bytes(r.tobytes(), "little") for r in k.reshape(-1, 32).cpu().numpy()]
    w = gc.expect_threads(oracle, x.reshape(-1, GT).cpu().numpy(), kint, table, False)
    assert (got.cpu().numpy() == w).all()
    # products only, and segments that are not equal (the pieces of the short ones are empty or one factor long)
    prod = eng.gt_prod(x.reshape(-1), table)
    assert bool((prod == fold_mul(eng, x, n_seg, m)).all())
    uneven = [0, 3, 3, 2 * m + 1, 4 * m]
    got_u = eng.gt_multi_exp(x.reshape(-1), k.reshape(-1), uneven).cpu().numpy()
    e = eng.gt_exp(x.reshape(-1), k.reshape(-1))
    one = to_dev(gc.pool(oracle)["one"])
    pad = lambda t, size: torch.cat([t, one.expand(size - t.shape[0], GT)])
    big = 1 << 18
    want_u = [fold_mul(eng, pad(e[a:b], big if b - a > 4 else 4), 1, big if b - a > 4 else 4)[0].cpu().numpy() for a, b in zip(uneven, uneven[1:])]
    assert (got_u == np.stack(want_u)).all()
    torch.cuda.synchronize()


def test_more_pieces_than_one_launch(eng, oracle):
    """65536 + 70000 segments of 0 .. 2 factors: two launches of 65536 pieces and a third; segment s is one, e_i or e_i e_(i+1)"""
    import torch
    n_seg = 65536 + 70000
    lengths = np.arange(n_seg) % 3
    seg = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(seg[-1])
    x, k = sized_inputs(eng, n, "chunks")
    got = eng.gt_multi_exp(x.reshape(-1), k.reshape(-1), seg.astype(np.uint64))
    e = eng.gt_exp(x.reshape(-1), k.reshape(-1))
    one = to_dev(gc.pool(oracle)["one"])
    e1 = torch.cat([e, one, one])
    lo = to_dev(seg[:-1])
    L = to_dev(lengths)
    first = torch.where((L >= 1).reshape(-1, 1), e1[lo], one.expand(n_seg, GT))
    second = torch.where((L >= 2).reshape(-1, 1), e1[lo + 1], one.expand(n_seg, GT))
    want = eng.gt_mul(first.contiguous().reshape(-1), second.contiguous().reshape(-1))
    wrong = torch.nonzero((got != want).any(dim=1)).flatten()
    assert wrong.numel() == 0, wrong[:8].tolist()
    for s in (65534, 65535, 65536, 65537, 131071, 131072, n_seg - 1):
        a, b = int(seg[s]), int(seg[s + 1])
        kint = [int.from_bytes(r.tobytes(), "little") for r in k.reshape(-1, 32)[a:b].cpu().numpy()]
        w = gc.expect(oracle, x.reshape(-1, GT)[a:b].cpu().numpy(), kint, [0, b - a], False)
        assert (got[s].cpu().numpy() == w[0]).all(), s


def test_caller_buffers_and_workspace(eng, oracle):
    import torch
    p = gc.pool(oracle)
    x, k, seg = gc.take(p["pair"], 40), gc.rand_exps("bufs", 40), [0, 10, 40]
    want = gc.expect(oracle, x, k, seg, False)
    wsb = eng._lib.load().gpbc_gt_multi_exp_workspace_bytes(40, 2)
    ws = torch.zeros(wsb + 512, dtype=torch.uint8, device="cuda")
    buf = torch.full((3 * GT,), 0x5A, dtype=torch.uint8, device="cuda")
    out = eng.gt_multi_exp(to_dev(x.reshape(-1)), to_dev(gc.krows(k).reshape(-1)), seg, out=buf[:2 * GT], workspace=ws[:wsb])
    assert (out.cpu().numpy().reshape(2, GT) == want).all() and bool((buf[2 * GT:] == 0x5A).all()) and bool((ws[wsb:] == 0).all())
    h = np.zeros((2, GT), dtype=np.uint8)
    assert eng.gt_multi_exp(x.reshape(-1), k, seg, out=h) is h and (h == want).all()


def test_wrong_inputs_are_refused_before_a_launch(eng, oracle):
    import torch
    from gopairingbasedcryptography_amd import EngineError
    p = gc.pool(oracle)
    x, k = to_dev(gc.take(p["pair"], 6).reshape(-1)), to_dev(gc.krows(gc.rand_exps("bad", 6)).reshape(-1))
    t = lambda *v: to_dev(np.array(v, dtype=np.int64))
    for table in (t(0, 4, 3, 6), t(1, 3, 6), t(0, 3, 5), t(0, 3, 7)):                  # a device table is validated on the device
        with pytest.raises(ValueError):
            eng.gt_multi_exp(x, k, table)
    with pytest.raises(ValueError):
        eng.gt_multi_exp(x, k[:3 * 32].contiguous(), t(0, 2, 6))                        # shared list of 3, segments of 2 and 4
    with pytest.raises(ValueError):
        eng.gt_multi_exp(x, k, [0, 6], workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        eng.gt_multi_exp(x, k, [0, 6], out=torch.zeros(GT, dtype=torch.uint8))          # out on the host
    with pytest.raises(EngineError):
        eng.gt_multi_exp(x, k, [0, 3, 6], out=x[:2 * GT])                               # out overlaps x: refused by the C entry
    lib = eng._lib.load()
    seg = np.array([0, 3, 6], dtype=np.uint64)
    hx, hk, ho = x.cpu().numpy(), k.cpu().numpy(), np.zeros(2 * GT, np.uint8)
    import ctypes
    VP, SZ = (lambda a: ctypes.c_void_p(a.ctypes.data)), ctypes.c_size_t
    assert lib.gpbc_gt_multi_exp(VP(hx), VP(hk), SZ(5), VP(seg), SZ(2), VP(ho)) == -1 and b"nk" in lib.gpbc_last_error()
    assert lib.gpbc_gt_multi_exp(VP(hx), VP(hk), SZ(6), VP(seg), SZ(2), VP(hx)) == -1 and b"overlap" in lib.gpbc_last_error()
    assert not ho.any()
    torch.cuda.synchronize()
    assert bool((eng.gt_multi_exp(x, k, [0, 6]) == eng.gt_multi_exp(x, k, t(0, 6))).all())       # the engine is fine afterwards
