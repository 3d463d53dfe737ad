"""Segmented G1 / G2 multi-scalar multiplication on the MI355X (run with -m gpu): k_g*_multi_scalar_mul / k_g*_sum_segments through
the host-pointer and the device entries of include/gpbc_bn254_ext.h.

  * the case lists of tests/gmsm_cases.py against the oracle (scalar multiplication per term, summed per segment), bit for bit: host
    arrays, CUDA tensors with the table on the host and on the device, caller buffers with guard bytes on both sides, and once more
    in a process bound to the device list {0, 0} with calls large enough to cross the shard split (whole segments per shard);
  * agreement of forms, bit for bit (canonical outputs leave no tolerance): fr_lsss_weights -> fr_neg -> g1_multi_scalar_mul against
    g1_scalar_mul folded with g1_add; more pieces than one launch takes;
  * the stream contract of the two _dev entries with the gate and the decoys of tests/test_stream_contract_gpu.py;
  * wrong inputs are refused on the host before anything is launched on them."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT
import gmsm_cases as gc
from test_host_device_forms_gpu import Offsets, arguments, results
from test_stream_contract_gpu import Recorder, Rig, prepare, same_bytes

pytestmark = pytest.mark.gpu
GROUPS = [False, True]
IDS = ["g1", "g2"]


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def entries(eng, g2):
    return (eng.g2_multi_scalar_mul, eng.g2_sum_segments, eng.g2_scalar_mul, eng.g2_add) if g2 else (eng.g1_multi_scalar_mul, eng.g1_sum_segments, eng.g1_scalar_mul, eng.g1_add)


def fold_add(add, e, n_seg, m, w):
    """sum over the m columns of e [n_seg * m, w] with the engine's elementwise addition: log2(m) rounds (m a power of two)"""
    cur = e.reshape(n_seg, m, w)
    while m > 1:
        cur = add(cur[:, 0::2].contiguous().reshape(-1), cur[:, 1::2].contiguous().reshape(-1)).reshape(n_seg, m // 2, w)
        m //= 2
    return cur.reshape(n_seg, w)


@pytest.mark.parametrize("g2", GROUPS, ids=IDS)
def test_cases_host_and_device(eng, oracle, g2):
    import torch
    assert gc.run_engine_cases(eng, oracle, g2) == []
    assert gc.run_engine_cases(eng, oracle, g2, put=to_dev) == []
    assert gc.run_engine_cases(eng, oracle, g2, put=to_dev, table_on_device=True) == []
    torch.cuda.synchronize()


@pytest.mark.parametrize("g2", GROUPS, ids=IDS)
def test_cases_into_caller_buffers_with_guards(eng, oracle, g2):
    """every case into a caller's output and workspace that sit inside larger buffers: the bytes on both sides stay as they were"""
    import torch
    msm, _, _, _ = entries(eng, g2)
    w, guard = gc.BYTES[g2], 512
    want_all = gc.expected(oracle, g2)
    lib = eng._lib.load()
    for label, x, k, seg, shared in gc.cases(g2):
        n, n_seg = len(x), len(seg) - 1
        wsb = max(lib.gpbc_multi_scalar_mul_workspace_bytes(n, n_seg, int(g2)), 1)
        ws = torch.full((wsb + 2 * guard,), 0xC3, dtype=torch.uint8, device="cuda")
        buf = torch.full((n_seg * w + 2 * guard,), 0x5A, dtype=torch.uint8, device="cuda")
        out = msm(to_dev(np.ascontiguousarray(x).reshape(-1)), None if k is None else to_dev(gc.krows(k).reshape(-1)), to_dev(np.array(seg, dtype=np.int64)),
                  out=buf[guard:guard + n_seg * w], workspace=ws[guard:guard + wsb])
        assert (out.cpu().numpy().reshape(n_seg, w) == want_all[label]).all(), label
        assert bool((buf[:guard] == 0x5A).all()) and bool((buf[guard + n_seg * w:] == 0x5A).all()), label
        assert bool((ws[:guard] == 0xC3).all()) and bool((ws[guard + wsb:] == 0xC3).all()), label
    x, k, seg = gc.take(gc.pool(g2)["pt"], 10), gc.rand_scalars("hostbuf", 10), [0, 3, 10]
    h = np.full((4, w), 0x5A, dtype=np.uint8)
    assert (msm(x.reshape(-1), k, seg, out=h[1:3]) == gc.expect(oracle, g2, x, k, seg, False)).all() and (h[0] == 0x5A).all() and (h[3] == 0x5A).all()


def test_host_entry_across_the_shard_split():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gmsm_cases.py"), "0", "0"], capture_output=True, text=True, timeout=900)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "devices 2 failures []" in r.stdout


def test_lsss_weights_chain_equals_the_composed_route(eng, oracle):
    """fr_lsss_weights -> fr_neg -> g1_multi_scalar_mul on device buffers, nothing leaving HBM, against g1_scalar_mul + rounds of g1_add"""
    import torch
    n, R, C = 96, 4, 2
    r = eng.R_ORDER
    matrix = eng.fr_to_bytes([1, 1, 0, r - 1, 1, 2, 0, 1]).copy()                       # rows (1, 1), (0, -1), (1, 2), (0, 1)
    held = (np.arange(n * R).reshape(n, R) * 2654435761 >> 9 & 1).astype(np.uint8)
    held[::3] = (1, 1, 0, 0)
    w, ok = eng.fr_lsss_weights(to_dev(np.tile(matrix, n)), R, C, to_dev(held).reshape(-1))
    assert 0 < int(ok.sum()) <= n
    nw = eng.fr_neg(w.reshape(-1))
    cx = to_dev(eng.g1_scalar_mul_base(list(range(5, 5 + n * R))))
    table = np.arange(0, n * R + 1, R, dtype=np.uint64)
    got = eng.g1_multi_scalar_mul(cx.reshape(-1), nw.reshape(-1), to_dev(table.astype(np.int64)))
    want = fold_add(eng.g1_add, eng.g1_scalar_mul(cx.reshape(-1), nw.reshape(-1)), n, R, 64)
    assert bool((got == want).all())
    kint = eng.fr_to_ints(nw)
    assert (got.cpu().numpy() == gc.expect(oracle, False, cx.cpu().numpy(), kint, [int(v) for v in table], False)).all()
    torch.cuda.synchronize()


def test_more_pieces_than_one_launch(eng, oracle):
    """131072 + 5000 segments of 0 .. 2 terms: one full launch of 131072 pieces and a second; segment s is infinity, t_i or t_i + t_(i+1)"""
    import torch
    n_seg = gc.FILL + 5000
    lengths = np.arange(n_seg) % 3
    seg = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(seg[-1])
    rng = np.random.default_rng(gc.hash_tag("chunks"))
    x = to_dev(eng.g1_scalar_mul_base(list(range(1, 4097))))[torch.arange(n, device="cuda") % 4096].contiguous()
    k = to_dev(rng.integers(0, 256, size=(n, 32), dtype=np.uint8))
    got = eng.g1_multi_scalar_mul(x.reshape(-1), k.reshape(-1), seg.astype(np.uint64))
    e = torch.cat([eng.g1_scalar_mul(x.reshape(-1), k.reshape(-1)), torch.zeros((2, 64), dtype=torch.uint8, device="cuda")])
    lo, L = to_dev(seg[:-1]), to_dev(lengths)
    zero = torch.zeros((n_seg, 64), dtype=torch.uint8, device="cuda")
    first = torch.where((L >= 1).reshape(-1, 1), e[lo], zero)
    second = torch.where((L >= 2).reshape(-1, 1), e[lo + 1], zero)
    want = eng.g1_add(first.contiguous().reshape(-1), second.contiguous().reshape(-1))
    wrong = torch.nonzero((got != want).any(dim=1)).flatten()
    assert wrong.numel() == 0, wrong[:8].tolist()
    for s in (gc.FILL - 2, gc.FILL - 1, gc.FILL, gc.FILL + 1, n_seg - 1):
        a, b = int(seg[s]), int(seg[s + 1])
        kint = [int.from_bytes(r.tobytes(), "little") for r in k[a:b].cpu().numpy()]
        assert (got[s].cpu().numpy() == gc.expect(oracle, False, x[a:b].cpu().numpy(), kint, [0, b - a], False)[0]).all(), s


# ------------------------------------------------------------------------------------------------ the stream contract of the _dev entries
def dev_entry(eng, g2):
    """fn(bases, scalars | None, table): numpy arguments go through the wrapper's host form (the expected answer); CUDA tensors go to
    the C entry gpbc_g*_multi_scalar_mul_dev itself on the current stream, with an output and a workspace made before the gate —
    a device table as it is, a host table (a list) copied to the device once, outside the call under test"""
    import torch
    from gopairingbasedcryptography_amd import _lib
    w = gc.BYTES[g2]
    msm = eng.g2_multi_scalar_mul if g2 else eng.g1_multi_scalar_mul
    name = "gpbc_g2_multi_scalar_mul_dev" if g2 else "gpbc_g1_multi_scalar_mul_dev"
    keep = {}

    def fn(bases, scalars, table):
        if isinstance(bases, np.ndarray):
            return msm(bases.reshape(-1), None if scalars is None else scalars.reshape(-1), table)
        if not torch.is_tensor(table):
            key = tuple(int(v) for v in table)
            if key not in keep:
                keep[key] = torch.tensor(key, dtype=torch.int64).cuda()
                torch.cuda.synchronize()
            table = keep[key]
        n, n_seg = bases.numel() // w, table.numel() - 1
        nk = 0 if scalars is None else scalars.numel() // 32
        lib = _lib.load()
        size = max(lib.gpbc_multi_scalar_mul_workspace_bytes(n, n_seg, int(g2)), 1)
        if (n, n_seg) not in keep:
            keep[(n, n_seg)] = (torch.empty((n_seg, w), dtype=torch.uint8, device="cuda"), torch.empty(size, dtype=torch.uint8, device="cuda"))
        out, ws = keep[(n, n_seg)]
        _lib.check(getattr(lib, name)(bases.data_ptr(), None if scalars is None else scalars.data_ptr(), nk, table.data_ptr(), n, n_seg, out.data_ptr(),
                                      ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
        return out
    return fn


def tag(g2):
    return "g2" if g2 else "g1"


def contract_cases(eng, g2):
    """(label, fn, arguments): the three forms of the scalars, each with the table on the host and on the device; 11 terms in segments
    of 5 / 0 / 6 (more than one group per lane), 12 in three segments of 4 for the shared list, and one segment of 40 that is cut
    into pieces and folded"""
    p = gc.pool(g2)
    fn = dev_entry(eng, g2)
    t = tag(g2)
    x11, x12, x40 = gc.take(p["pt"], 11), gc.take(p["pt"], 12, 3), gc.take(np.concatenate([p["pt"], p["neg"][:5]]), 40)
    k11, k4, k40 = gc.krows(gc.rand_scalars(t + "c11", 11)), gc.krows(gc.rand_scalars(t + "c4", 4)), gc.krows(gc.rand_scalars(t + "c40", 40))
    for how, tab in (("host table", lambda v: v), ("device table", Offsets)):
        yield "%s one scalar per term, %s" % (t, how), fn, (x11, k11, tab([0, 5, 5, 11]))
        yield "%s one list, %s" % (t, how), fn, (x12, k4, tab([0, 4, 8, 12]))
        yield "%s plain sums, %s" % (t, how), fn, (x11, None, tab([0, 5, 5, 11]))
        yield "%s one segment of 40, %s" % (t, how), fn, (x40, k40, tab([0, 40]))
        yield "%s sum of 40, %s" % (t, how), fn, (x40, None, tab([0, 40]))


@pytest.fixture(scope="module")
def rig(eng):
    return Rig(eng)


@pytest.mark.parametrize("g2", GROUPS, ids=IDS)
def test_dev_entries_are_ordered_behind_the_stream_and_do_not_wait(eng, rig, oracle, g2):
    """The gated procedure of test_stream_contract_gpu.run_family on the C entries themselves: the arguments hold a decoy, the real
    inputs arrive behind a gate on a side stream, the decoy comes back after the call.  The call must return with the gate still
    closed (it does not wait for the stream), its result must be the host form's answer on the real inputs (every kernel ran on that
    stream, behind the copies: a kernel on the null stream would have read the decoy), and equal the oracle."""
    from gopairingbasedcryptography_amd import _lib
    torch, s = rig.torch, rig.streams[0]
    wrong, work = [], []
    for label, fn, args in contract_cases(eng, g2):
        # (the decoy rules go by the label: a whole-array sum is the same on rolled rows, so there the decoy also loses a row)
        want, decoy, other = prepare("g_sum" if label.startswith(tag(g2) + " sum of") else "g_multi_scalar_mul", fn, args)
        if same_bytes(want, other):
            wrong.append("%s: the decoy gives the same answer as the real inputs" % label)
        table = args[2].values if isinstance(args[2], Offsets) else args[2]
        ks = None if args[1] is None else [int.from_bytes(r.tobytes(), "little") for r in args[1]]
        if not (want[0] == gc.expect(oracle, g2, args[0], ks, table, ks is not None and len(ks) != len(args[0]))).all():
            wrong.append("%s: the host form differs from the oracle" % label)
        real_d, decoy_d = arguments(args, True), arguments(decoy, True)
        slots = [i for i, a in enumerate(real_d) if torch.is_tensor(a)]
        live = list(real_d)
        for i in slots:
            live[i] = decoy_d[i].clone()
        work.append((label, fn, want, other, real_d, decoy_d, slots, live))
    torch.cuda.synchronize()

    def one(item, gate_ms):
        label, fn, _, _, real_d, decoy_d, slots, live = item
        with torch.cuda.stream(s):
            if gate_ms:
                rig.gate(gate_ms)
            for i in slots:
                live[i].copy_(real_d[i], non_blocking=True)
            filled = torch.cuda.Event()
            filled.record(s)
            t0 = time.perf_counter()
            res = results(fn(*live))
            dt = (time.perf_counter() - t0) * 1e3
            closed = not filled.query()
            snaps = [r.clone() for r in res]
            for i in slots:
                live[i].copy_(decoy_d[i], non_blocking=True)
        s.synchronize()
        return dt, closed, snaps

    slowest = 0.0
    for timed in (False, True):
        for item in work:                                         # workspaces and the allocator's blocks are warm after the first pass
            dt = one(item, 0)[0]
            if timed:
                slowest = max(slowest, dt)
    gate_ms = min(max(10 * slowest, 20.0), 250.0)
    seen = set()
    real_lib = _lib._lib
    _lib._lib = Recorder(real_lib, seen)
    try:
        for item in work:
            label, _, want, other = item[:4]
            dt, closed, snaps = one(item, gate_ms)
            got = [t.cpu().numpy() for t in snaps]
            print("  %-44s returned in %8.3f ms, gate of %.0f ms %s" % (label, dt, gate_ms, "closed" if closed else "open"))
            if not closed:
                wrong.append("%s: returned after %.3f ms with the gate of %.0f ms already open: it waited for the stream" % (label, dt, gate_ms))
            if not same_bytes(want, got):
                wrong.append("%s: the gated result differs from the host form on the real inputs%s" % (label, " and equals the answer on the decoy" if same_bytes(other, got) else ""))
    finally:
        _lib._lib = real_lib
    assert seen == {"gpbc_g2_multi_scalar_mul_dev" if g2 else "gpbc_g1_multi_scalar_mul_dev"}, seen
    assert not wrong, "\n".join(wrong)


def test_wrong_inputs_are_refused_before_a_launch(eng, oracle):
    import torch
    from gopairingbasedcryptography_amd import EngineError
    for g2 in GROUPS:
        msm, plain, _, _ = entries(eng, g2)
        w = gc.BYTES[g2]
        p = gc.pool(g2)
        x, k = to_dev(gc.take(p["pt"], 6).reshape(-1)), to_dev(gc.krows(gc.rand_scalars("bad", 6)).reshape(-1))
        t = lambda *v: to_dev(np.array(v, dtype=np.int64))
        for table in (t(0, 4, 3, 6), t(1, 3, 6), t(0, 3, 5), t(0, 3, 7)):                  # a device table is validated on the device
            with pytest.raises(ValueError):
                msm(x, k, table)
        with pytest.raises(ValueError):
            msm(x, k[:3 * 32].contiguous(), t(0, 2, 6))                                     # shared list of 3, segments of 2 and 4
        with pytest.raises(ValueError):
            msm(x, k, [0, 6], workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError):
            msm(x, k, [0, 6], out=torch.zeros(w, dtype=torch.uint8))                        # out on the host
        big = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError):
            msm(x, k, [0, 6], workspace=big[4:])                                            # workspace not 16-byte aligned
        with pytest.raises(EngineError):
            msm(x, k, [0, 3, 6], out=x[:2 * w])                                             # out overlaps the bases: refused by the C entry
        torch.cuda.synchronize()
        assert bool((msm(x, k, [0, 6]) == msm(x, k, t(0, 6))).all())                        # the engine is fine afterwards
        assert bool((plain(x, [0, 2, 6]) == plain(x, t(0, 2, 6))).all())
