"""The XOR mask from GT bytes on the MI355X (run with -m gpu): gpbc_gt_xor_mask and gpbc_gt_xor_mask_dev through bn254.gt_xor_mask on
every case of tests/mask_cases.py — the host entry, the _dev entry on CUDA tensors, the row form, and in place — byte for byte against
the pure-Python expectation, with out_len exact and every byte of `out` that belongs to no message left as a canary fill wrote it;
against gt_marshal followed by a host XOR; whole pieces at every address path of the kernel; offsets the _dev form has to clamp; and
the stream contract of the _dev entry (the gated procedure of tests/test_stream_contract_gpu.py)."""
import numpy as np
import pytest

import mask_cases as mc

pytestmark = pytest.mark.gpu
FILL = 0x5C


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a, copy=True))
    return (t.to(dtype) if dtype is not None else t).cuda()


def filled_want(case):
    """the expectation for an `out` that was filled with FILL: the bytes no message owns keep it"""
    want = case["want"].copy()
    a, b = int(case["off"][0]), int(case["off"][-1])
    want[:a] = FILL
    want[b:] = FILL
    return want


def same(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    return got.shape == np.asarray(want).shape and got.tobytes() == np.asarray(want).tobytes()


def lens_ok(out_len, case, device):
    import torch
    if device:
        return isinstance(out_len, torch.Tensor) and out_len.is_cuda and out_len.dtype == torch.int32 and out_len.cpu().numpy().view(np.uint32).tolist() == case["want_len"].tolist()
    return isinstance(out_len, np.ndarray) and out_len.dtype == np.uint32 and out_len.tolist() == case["want_len"].tolist()


@pytest.mark.parametrize("case", mc.cases(), ids=mc.case_ids())
def test_every_form_is_byte_exact(eng, case):
    import torch
    gt, data, off = case["gt"].copy(), case["data"].copy(), case["off"].copy()
    # 1. the host entry: flat buffer plus offsets into a canary-filled out, then the list of bytes
    out = np.full(data.size, FILL, np.uint8)
    got, out_len = eng.gt_xor_mask(gt, data, off, out=out)
    assert got is out and same(out, filled_want(case)) and lens_ok(out_len, case, False)
    assert same(data, case["data"]) and same(gt, case["gt"])                               # the inputs are not written
    (flat, offs), out_len = eng.gt_xor_mask(gt, case["msgs"])
    a, b = int(off[0]), int(off[-1])
    assert same(flat, case["want"][a:b]) and offs.tolist() == [int(v) - a for v in off] and lens_ok(out_len, case, False)
    # 2. the _dev entry on CUDA tensors
    d_gt, d_data, d_off = dev(gt), dev(data), dev(off, torch.int64)
    d_out = torch.full((data.size,), FILL, dtype=torch.uint8, device="cuda")
    got, out_len = eng.gt_xor_mask(d_gt, d_data, d_off, out=d_out)
    assert got is d_out and same(d_out, filled_want(case)) and lens_ok(out_len, case, True)
    assert same(d_data, case["data"]) and same(d_gt, case["gt"])
    got, out_len = eng.gt_xor_mask(d_gt, d_data, d_off)                                    # an output made by the call
    assert got.is_cuda and same(got[a:b], case["want"][a:b]) and lens_ok(out_len, case, True)
    # 3. in place, host and device: the message buffer is the output, the canaries around the messages stay
    buf = data.copy()
    got, out_len = eng.gt_xor_mask(gt, buf, off, out=buf)
    assert got is buf and same(buf, case["want"]) and lens_ok(out_len, case, False)
    d_buf = dev(data)
    got, out_len = eng.gt_xor_mask(d_gt, d_buf, d_off, out=d_buf)
    assert got is d_buf and same(d_buf, case["want"]) and lens_ok(out_len, case, True)
    # 4. the row form of a row case, the same four ways
    if case["width"] is not None:
        rows, want = mc.rows_of(case)
        got, out_len = eng.gt_xor_mask(gt, rows.copy())
        assert same(got, want) and lens_ok(out_len, case, False)
        got, out_len = eng.gt_xor_mask(d_gt, dev(rows))
        assert got.is_cuda and same(got, want) and lens_ok(out_len, case, True)
        buf, d_buf = rows.copy(), dev(rows)
        assert eng.gt_xor_mask(gt, buf, out=buf)[0] is buf and same(buf, want)
        assert eng.gt_xor_mask(d_gt, d_buf, out=d_buf)[0] is d_buf and same(d_buf, want)
    # ... and what it replaces on the same inputs: gt_marshal, then XOR on the host
    marshalled = eng.gt_marshal(gt)
    for m, row, want_len, lo in zip(case["msgs"], marshalled, case["want_len"], off[:-1]):
        L = int(want_len)
        assert bytes(x ^ y for x, y in zip(m[:L], row.tobytes())) == case["want"][int(lo):int(lo) + L].tobytes()


@pytest.mark.parametrize("shift", [1, 4, 16, 48])
def test_whole_pieces_at_every_address_path(eng, shift):
    """rows of 32 and the 65-item ragged batch placed `shift` bytes into a device buffer: odd, 4-byte and 16-byte addresses (a CUDA
    allocation starts on a 256-byte boundary), out at the same shift and, for the mixed paths, at another"""
    import torch
    for case in (mc.cases()[3], mc.cases()[5]):
        assert case["label"] in ("ragged-65", "rows-32")
        size = case["data"].size
        d_gt, d_off = dev(case["gt"]), dev(case["off"], torch.int64)
        for out_shift in sorted({shift, 16}):
            msgs = torch.full((size + 64,), FILL, dtype=torch.uint8, device="cuda")
            out = torch.full((size + 64,), FILL, dtype=torch.uint8, device="cuda")
            msgs[shift:shift + size] = dev(case["data"])
            view_in, view_out = msgs[shift:shift + size], out[out_shift:out_shift + size]
            assert view_in.data_ptr() % 256 == shift and view_out.data_ptr() % 256 == out_shift
            got, out_len = eng.gt_xor_mask(d_gt, view_in, d_off, out=view_out)
            assert same(view_out, filled_want(case)) and lens_ok(out_len, case, True)
            assert (out[:out_shift] == FILL).all() and (out[out_shift + size:] == FILL).all()
            if case["width"] is not None:                                                 # the row form at the same addresses
                n, w = case["n"], case["width"]
                out2 = torch.full((size + 64,), FILL, dtype=torch.uint8, device="cuda")
                rows_out = out2[out_shift:out_shift + size].view(n, w)
                eng.gt_xor_mask(d_gt, view_in.view(n, w), out=rows_out)
                assert same(rows_out, mc.rows_of(case)[1]) and (out2[:out_shift] == FILL).all() and (out2[out_shift + size:] == FILL).all()


def test_device_offsets_are_clamped(eng):
    """a malformed device-resident table: an offset far past the buffer acts as its end, a decreasing pair is an empty message; nothing
    outside the 64 bytes is read or written"""
    import torch
    kinds = [2, 3, 2, 4]
    gt = np.stack([mc.KINDS[k][1] for k in kinds])
    body = np.frombuffer(mc.message("clamp", 0, 64), dtype=np.uint8).copy()
    big_in = torch.full((128,), FILL, dtype=torch.uint8, device="cuda")
    big_out = torch.full((128,), FILL, dtype=torch.uint8, device="cuda")
    big_in[:64] = dev(body)
    off = torch.tensor([0, 24, 24, 10 ** 12, 50], dtype=torch.int64).cuda()
    got, out_len = eng.gt_xor_mask(dev(gt), big_in[:64], off, out=big_out[:64])
    want = mc.xor_cut(body[:24].tobytes(), mc.KINDS[2][2])[0] + mc.xor_cut(body[24:].tobytes(), mc.KINDS[2][2])[0]
    assert big_out[:64].cpu().numpy().tobytes() == want and (big_out[64:] == FILL).all()
    assert out_len.cpu().numpy().tolist() == [24, 0, 40, 0]


def test_dev_form_is_ordered_on_the_callers_stream_and_does_not_wait(eng):
    """the gated procedure of tests/test_stream_contract_gpu.py: the _dev call enqueued on a side stream sees the producer's output —
    the real inputs, copied in behind a closed gate — and returns while the gate is closed"""
    import test_stream_contract_gpu as contract
    rig = contract.Rig(eng)
    rows_case, ragged = mc.cases()[6], mc.cases()[2]
    assert rows_case["label"] == "rows-33" and ragged["label"] == "ragged-22"
    rows, _ = mc.rows_of(rows_case)
    a, b = int(ragged["off"][0]), int(ragged["off"][-1])                                   # the messages alone: every byte of the output is then defined
    case_list = [
        ("gt_xor_mask rows", lambda gt, m: eng.gt_xor_mask(gt, m), (rows_case["gt"].copy(), rows.copy()), None),
        ("gt_xor_mask ragged", lambda gt, m, off: eng.gt_xor_mask(gt, m, off), (ragged["gt"].copy(), ragged["data"][a:b].copy(), contract.Offsets([int(v) - a for v in ragged["off"]])), None),
    ]
    wrong = contract.run_family(rig, "mask", case_list)
    assert not wrong, "\n".join(wrong)
    assert "gpbc_gt_xor_mask_dev" in rig.seen
