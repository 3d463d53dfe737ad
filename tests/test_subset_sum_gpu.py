"""Bit-selected sums over a fixed set on the device (run with -m gpu): the case list of subset_cases.py through bn254.SubsetTable for G1
and G2 with host arrays and with CUDA tensors, random 256-bit masks at the batch sizes around a wavefront, the chunked route (2 048 bits,
3 items; the cap, 16 384 bits) with its workspace, two tables alive at once, and the stream contract of the two device entries: a
table built on a side stream and used there without a synchronise in between, and a sum behind a slow predecessor on its stream.
Every expected point is the oracle's sum over [O] + the selected bases; comparisons are byte for byte."""
import ctypes

import numpy as np
import pytest

import subset_cases as sc
from test_stream_contract_gpu import Rig

pytestmark = pytest.mark.gpu
GROUPS = [False, True]
IDS = ["g1", "g2"]
GATE_MS = 50.0


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


@pytest.fixture(scope="module")
def rig(eng):
    return Rig(eng)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("g2", GROUPS, ids=IDS)
def test_case_list_host_arrays(eng, oracle, g2):
    want = sc.expected(oracle, g2)
    bad = []
    for t in sc.tables(oracle, g2):
        table = eng.SubsetTable(t.B, offset=t.O, g2=g2)
        assert table.nbits == t.nbits and table.table_bytes() == (t.nbits + 7) // 8 * 256 * (257 if g2 else 129)
        got = table.sum(t.masks)
        table.close()
        if not (got == want[t.label]).all():
            bad.append((t.label, [t.names[i] for i in np.nonzero((got != want[t.label]).any(axis=1))[0][:6]]))
    assert not bad, bad


@pytest.mark.parametrize("g2", GROUPS, ids=IDS)
def test_case_list_cuda_tensors(eng, oracle, g2):
    import torch
    want = sc.expected(oracle, g2)
    bad = []
    for t in sc.tables(oracle, g2):
        table = eng.SubsetTable(dev(t.B), offset=None if t.O is None else dev(t.O), g2=g2)
        got = table.sum(dev(t.masks))
        assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (len(t.masks), sc.BYTES[g2])
        got = host(got)
        table.close()
        if not (got == want[t.label]).all():
            bad.append((t.label, [t.names[i] for i in np.nonzero((got != want[t.label]).any(axis=1))[0][:6]]))
    assert not bad, bad


@pytest.fixture(scope="module")
def random_256(oracle):
    """per group: the table rand/point/256 with 1 000 random masks and the oracle's sums, computed once"""
    out = {}
    for g2 in GROUPS:
        t = sc.make_table(oracle, g2, "rand", "point", 256)
        masks = sc.random_masks("gpu-256-%d" % g2, 1000, 32)
        out[g2] = (t, masks, sc.expect(oracle, g2, t, masks))
    return out


@pytest.mark.parametrize("g2", GROUPS, ids=IDS)
def test_random_masks_around_a_wavefront(eng, random_256, g2):
    t, masks, want = random_256[g2]
    table = eng.SubsetTable(t.B, offset=t.O, g2=g2)
    for n in (1, 63, 64, 65, 1000):
        assert table.workspace_bytes(n) == 0                                   # 32 windows: one chunk whatever n is
        assert (table.sum(masks[:n]) == want[:n]).all(), n
        assert (host(table.sum(dev(masks[:n]))) == want[:n]).all(), n
    # an [n, 256] array of 0 / 1 is packed by the wrapper; out= is written in place, on either side
    assert (table.sum(np.unpackbits(masks[:65], axis=1)) == want[:65]).all()
    out = np.zeros((65, sc.BYTES[g2]), dtype=np.uint8)
    assert table.sum(masks[:65], out=out) is out and (out == want[:65]).all()
    d_out = dev(np.zeros((65, sc.BYTES[g2]), dtype=np.uint8))
    assert table.sum(dev(masks[:65]), out=d_out) is d_out and (host(d_out) == want[:65]).all()
    assert table.sum(masks[:0]).shape == (0, sc.BYTES[g2])                     # n = 0: a no-op
    one_shot = (eng.g2_subset_sum if g2 else eng.g1_subset_sum)
    assert (one_shot(t.B, masks[:5], offset=t.O) == want[:5]).all()
    assert (host(one_shot(dev(t.B), dev(masks[:5]), offset=dev(t.O))) == want[:5]).all()
    table.close()
    with pytest.raises(ValueError):
        table.sum(masks[:1])                                                   # closed


@pytest.mark.parametrize("g2", GROUPS, ids=IDS)
@pytest.mark.parametrize("nbits", [2048, sc.MAX_BITS])
def test_chunked_route_and_its_workspace(eng, oracle, g2, nbits):
    """3 bitmaps of 2 048 bits: 8 chunks of 32 windows, partial sums chunk-major in the workspace, one fold; the cap: 64 chunks"""
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    W, pt = nbits // 8, sc.BYTES[g2]
    t = sc.make_table(oracle, g2, "rand", "point", nbits, extra_masks=sc.random_masks("chunked-%d-%d" % (nbits, g2), 2, W))
    masks = t.masks[[t.row("ones"), t.row("extra 0"), t.row("extra 1")]]
    want = sc.expect(oracle, g2, t, masks)
    table = eng.SubsetTable(dev(t.B), offset=dev(t.O), g2=g2)
    need = table.workspace_bytes(3)
    assert need == (W // 32) * 3 * pt > 0
    assert (table.sum(masks) == want).all()
    assert (host(table.sum(dev(masks))) == want).all()
    ws = dev(np.zeros(need, dtype=np.uint8))
    assert (host(table.sum(dev(masks), workspace=ws)) == want).all() and host(ws).any()        # the caller's workspace is the one used
    with pytest.raises(ValueError):
        table.sum(dev(masks), workspace=ws[:need - 1])
    # the C entry: a short or a missing workspace is GPBC_ERR_INVALID_ARG before any launch, nothing written
    d_masks, d_out = dev(masks), dev(np.full((3, pt), 0xA5, dtype=np.uint8))
    for args in ((ws.data_ptr(), need - 1), (None, need), (None, 0)):
        assert lib.gpbc_subset_sum_dev(table._h, d_masks.data_ptr(), 3, d_out.data_ptr(), args[0], args[1], None) == -1
        assert b"workspace" in lib.gpbc_last_error()
    assert lib.gpbc_subset_sum_dev(table._h, None, 3, d_out.data_ptr(), ws.data_ptr(), need, None) == -1
    assert lib.gpbc_subset_sum_dev(table._h, d_masks.data_ptr(), 3, None, ws.data_ptr(), need, None) == -1
    assert lib.gpbc_subset_sum_dev(table._h, None, 0, None, None, 0, None) == 0                  # n = 0
    assert (host(d_out) == 0xA5).all()
    table.close()


def test_two_tables_alive_at_once(eng, oracle, random_256):
    t1, masks, want1 = random_256[True]
    t2 = sc.make_table(oracle, False, "holes", "-B0", 257)
    a, b = eng.SubsetTable(t1.B, offset=t1.O, g2=True), eng.SubsetTable(dev(t2.B), offset=dev(t2.O), g2=False)
    want2 = sc.expected(oracle, False)[t2.label]
    for _ in range(2):
        assert (a.sum(masks[:70]) == want1[:70]).all() and (b.sum(t2.masks) == want2).all()
        assert (host(b.sum(dev(t2.masks))) == want2).all() and (host(a.sum(dev(masks[:70]))) == want1[:70]).all()
    a.close()
    assert (b.sum(t2.masks) == want2).all()                                    # closing one leaves the other
    b.close()


@pytest.mark.parametrize("g2", GROUPS, ids=IDS)
def test_table_built_and_used_on_a_side_stream(eng, rig, random_256, g2):
    """create_dev enqueues the build on the caller's stream and returns; the sum on the same stream follows it with no synchronise in
    between.  The bases hold a decoy until a gate on that stream has passed, and again afterwards: a build on any other stream, or a
    sum that overtakes the build, gives other bytes."""
    torch = rig.torch
    t, masks, want = random_256[g2]
    real_B, real_O = dev(t.B), dev(t.O)
    B, O, d_masks = dev(np.roll(t.B, 1, axis=0)), dev(t.B[5]), dev(masks[:100])
    s = rig.streams[0]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        rig.gate(GATE_MS)
        B.copy_(real_B)
        O.copy_(real_O)
        table = eng.SubsetTable(B, offset=O, g2=g2)
        got = table.sum(d_masks).clone()
        B.copy_(real_B.roll(1, 0))
        O.zero_()
    s.synchronize()
    assert (host(got) == want[:100]).all()
    assert (host(table.sum(d_masks)) == want[:100]).all()                      # the table does not depend on the bases any more
    table.close()


@pytest.mark.parametrize("g2", GROUPS, ids=IDS)
@pytest.mark.parametrize("nbits", [256, 2048])
def test_sum_is_ordered_behind_a_slow_predecessor(eng, rig, oracle, random_256, g2, nbits):
    """gpbc_subset_sum_dev (one chunk, and chunked with the fold) reads its masks behind the earlier work of its stream and returns
    without waiting for it"""
    torch = rig.torch
    if nbits == 256:
        t, masks, want = random_256[g2]
        masks, want = masks[:200], want[:200]
    else:
        t = sc.make_table(oracle, g2, "rand", "none", nbits)
        masks = sc.random_masks("order-%d" % g2, 5, nbits // 8)
        want = sc.expect(oracle, g2, t, masks)
    table = eng.SubsetTable(t.B, offset=t.O, g2=g2)
    assert (table.workspace_bytes(len(masks)) > 0) == (nbits == 2048)
    real, arg = dev(masks), dev(np.roll(masks, 1, axis=0) ^ np.uint8(0x5A))
    table.sum(arg)                                                             # (the kernels are loaded before the timed part)
    s = rig.streams[1]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        rig.gate(GATE_MS)
        arg.copy_(real)
        filled = torch.cuda.Event()
        filled.record()
        got = table.sum(arg).clone()
        returned_early = not filled.query()
        arg.zero_()
    s.synchronize()
    assert (host(got) == want).all()
    assert returned_early, "gpbc_subset_sum_dev waited for the stream"
    table.close()


def test_c_entries_directly(eng, oracle, random_256):
    """create_dev / sum_dev / destroy without the wrapper, on the null stream; destroy drains the device, so the result is there"""
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    t, masks, want = random_256[False]
    B, d_masks = dev(t.B), dev(masks[:4])
    assert lib.gpbc_subset_table_create_dev(0, B.data_ptr(), 256, None, None, ctypes.byref(h)) == 0 and h.value
    out = dev(np.zeros((4, 64), dtype=np.uint8))
    assert lib.gpbc_subset_sum_workspace_bytes(h, 4) == 0
    assert lib.gpbc_subset_sum_dev(h, d_masks.data_ptr(), 4, out.data_ptr(), None, 0, None) == 0
    assert lib.gpbc_subset_table_destroy(h) == 0
    assert (host(out) == sc.expect(oracle, False, sc.Table("", t.B, None, 256, [], masks[:4]))).all()       # (no offset here)
