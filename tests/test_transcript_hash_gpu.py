"""The transcript hash H(u, v, w) and the plain SHA-256 on the device (run with -m gpu): the case lists of transcript_cases.py through
bn254.hash_g1_gt_gt_to_fr and bn254.sha256 with host arrays and with CUDA tensors, at the batch sizes around a wavefront and a
workgroup (1, 63, 64, 65, 257: the list rotated and tiled), with `out` given, with n = 0, and the stream contract of the two device
entries: on a side stream, behind a gate and behind the kernel that produces their inputs there, read after synchronising that stream
alone.  Every expected row is hashlib over the oracle's encodings; comparisons are bit for bit."""
import numpy as np
import pytest

import transcript_cases as tc
from test_stream_contract_gpu import Rig

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 257]
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


def bad_rows(got, want, names):
    return [names[i % len(names)] for i in np.nonzero((got != want).any(axis=1))[0][:8]]


# ------------------------------------------------------------------------------------------------ H(u, v, w)
def test_transcript_case_list_both_kinds(eng, oracle):
    import torch
    names, u, v, w, want = tc.transcript_arrays(oracle)
    got = eng.hash_g1_gt_gt_to_fr(u, v, w)
    assert isinstance(got, np.ndarray) and got.shape == want.shape and not bad_rows(got, want, names), bad_rows(got, want, names)
    got = eng.hash_g1_gt_gt_to_fr(dev(u), dev(v), dev(w))
    assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == want.shape and got.dtype == torch.uint8
    assert not bad_rows(host(got), want, names), bad_rows(host(got), want, names)


@pytest.mark.parametrize("n", SIZES)
def test_transcript_batch_sizes(eng, oracle, n):
    names, u, v, w, want = tc.transcript_arrays(oracle)
    shift = 7 * n
    names = [names[(i + shift) % len(names)] for i in range(len(names))]
    u, v, w, want = (tc.rotate(a, n, shift) for a in (u, v, w, want))
    got = eng.hash_g1_gt_gt_to_fr(u, v, w)
    assert got.shape == (n, 32) and not bad_rows(got, want, names), bad_rows(got, want, names)
    got = host(eng.hash_g1_gt_gt_to_fr(dev(u), dev(v), dev(w)))
    assert got.shape == (n, 32) and not bad_rows(got, want, names), bad_rows(got, want, names)


def test_transcript_out_given_and_nothing_to_do(eng, oracle):
    import torch
    _, u, v, w, want = tc.transcript_arrays(oracle)
    out = np.full((65, 32), 0xA5, dtype=np.uint8)
    assert eng.hash_g1_gt_gt_to_fr(u[:65], v[:65], w[:65], out=out) is out and (out == want[:65]).all()
    d_out = dev(np.full((65, 32), 0xA5, dtype=np.uint8))
    assert eng.hash_g1_gt_gt_to_fr(dev(u[:65]), dev(v[:65]), dev(w[:65]), out=d_out) is d_out and (host(d_out) == want[:65]).all()
    assert eng.hash_g1_gt_gt_to_fr(u[:0], v[:0], w[:0]).shape == (0, 32)
    empty = eng.hash_g1_gt_gt_to_fr(dev(u[:0]), dev(v[:0]), dev(w[:0]))
    assert isinstance(empty, torch.Tensor) and empty.is_cuda and tuple(empty.shape) == (0, 32)


def test_transcript_on_a_side_stream_behind_its_producer(eng, rig, oracle):
    """u and w arrive by copies, v is the result of a gt_mul launched on the same stream just before; all of it behind a gate, the
    decoys back afterwards, and only that stream is waited for"""
    torch = rig.torch
    _, u, v, w, want = tc.transcript_arrays(oracle)
    n = 80 + 32                                                                 # (every item; the last 32 are the random ones)
    one = np.frombuffer(tc.o.gt_to_bytes(tc.gt_edges(oracle)["one"]), dtype=np.uint8)
    real_u, real_w, real_v, ones = dev(u), dev(w), dev(v), dev(np.tile(one, (n, 1)))
    arg_u, arg_w, factor = dev(np.roll(u, 1, axis=0)), dev(np.roll(w, 3, axis=0)), dev(np.roll(v, 2, axis=0))
    eng.hash_g1_gt_gt_to_fr(arg_u, eng.gt_mul(factor, ones), arg_w)             # (the kernels are loaded before the gated part)
    s = rig.streams[0]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        rig.gate(GATE_MS)
        arg_u.copy_(real_u)
        arg_w.copy_(real_w)
        factor.copy_(real_v)
        filled = torch.cuda.Event()
        filled.record()
        produced = eng.gt_mul(factor, ones)                                     # v x 1: the same element, canonical bytes
        got = eng.hash_g1_gt_gt_to_fr(arg_u, produced, arg_w).clone()
        returned_early = not filled.query()
        arg_u.zero_()
        arg_w.zero_()
        factor.zero_()
    s.synchronize()
    assert (host(got) == want).all()                                           # (x 1 leaves all twelve coefficients as they are, zero and p - 1 too)
    assert returned_early, "gpbc_hash_g1_gt_gt_to_fr_dev waited for the stream"


# ------------------------------------------------------------------------------------------------ SHA-256
@pytest.mark.parametrize("to_fr", [False, True])
def test_sha256_case_list_every_message_form(eng, to_fr):
    import torch
    msgs = tc.sha_messages()
    want = tc.sha_expected(msgs, to_fr)
    got = eng.sha256(msgs, to_fr=to_fr)
    assert isinstance(got, np.ndarray) and (got == want).all(), [len(msgs[i]) for i in np.nonzero((got != want).any(axis=1))[0]]
    data, off = tc.flat_messages(msgs)
    assert (eng.sha256(data, off, to_fr=to_fr) == want).all()
    got = eng.sha256(dev(data), dev(off.astype(np.int64)), to_fr=to_fr)
    assert isinstance(got, torch.Tensor) and got.is_cuda and (host(got) == want).all()
    if not to_fr:
        for (m, hexdigest), row in zip(tc.KNOWN, host(got)[len(tc.SHA_LENGTHS):]):
            assert row.tobytes().hex() == hexdigest, m


@pytest.mark.parametrize("n", SIZES)
def test_sha256_batch_sizes(eng, n):
    base = tc.sha_messages()
    msgs = [base[(i + n) % len(base)] for i in range(n)]
    data, off = tc.flat_messages(msgs)
    for to_fr in (False, True):
        want = tc.sha_expected(msgs, to_fr)
        assert (eng.sha256(msgs, to_fr=to_fr) == want).all()
        assert (host(eng.sha256(dev(data), dev(off.astype(np.int64)), to_fr=to_fr)) == want).all()


def test_sha256_out_given_nothing_to_do_and_clamped_offsets(eng):
    import torch
    msgs = tc.sha_messages()
    data, off = tc.flat_messages(msgs)
    out = np.full((len(msgs), 32), 0xA5, dtype=np.uint8)
    assert eng.sha256(msgs, out=out) is out and (out == tc.sha_expected(msgs, False)).all()
    d_out = dev(np.full((len(msgs), 32), 0xA5, dtype=np.uint8))
    assert eng.sha256(dev(data), dev(off.astype(np.int64)), to_fr=True, out=d_out) is d_out and (host(d_out) == tc.sha_expected(msgs, True)).all()
    assert eng.sha256([]).shape == (0, 32)
    empty = eng.sha256(dev(data), dev(np.zeros(1, dtype=np.int64)))
    assert isinstance(empty, torch.Tensor) and empty.is_cuda and tuple(empty.shape) == (0, 32)
    # a device-resident table that points past the buffer is clamped to it (msg_range), as the hash-to-curve kernels clamp theirs
    three = [b"0123456789" * 7, b"abc", b"tail"]
    data3, off3 = tc.flat_messages(three)
    got = host(eng.sha256(dev(data3[:72]), dev(off3.astype(np.int64))))
    assert (got == tc.sha_expected([three[0], b"ab", b""], False)).all()


def test_sha256_on_a_side_stream_behind_its_producer(eng, rig):
    """the messages are written by a copy kernel on the same stream behind a gate; read after synchronising that stream alone"""
    torch = rig.torch
    msgs = tc.sha_messages() * 10
    data, off = tc.flat_messages(msgs)
    real, arg, d_off = dev(data), dev(data ^ np.uint8(0x5A)), dev(off.astype(np.int64))
    eng.sha256(arg, d_off, to_fr=True)
    s = rig.streams[1]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        rig.gate(GATE_MS)
        arg.copy_(real)
        filled = torch.cuda.Event()
        filled.record()
        got = eng.sha256(arg, d_off, to_fr=True).clone()
        returned_early = not filled.query()
        arg.zero_()
    s.synchronize()
    assert (host(got) == tc.sha_expected(msgs, True)).all()
    assert returned_early, "gpbc_sha256_batch_dev waited for the stream"


def test_identity_masks_on_the_device(eng):
    from gopairingbasedcryptography_amd import hash_to, waters05
    names = ["identity-%d@example.com" % i for i in range(70)] + [b"\x00", "x" * 300]
    want = waters05.identity_masks(names)
    assert (waters05.identity_masks_device(eng, names) == want).all()
    data, off = tc.flat_messages([n.encode() if isinstance(n, str) else n for n in names])
    got = waters05.identity_masks_device(eng, dev(data), dev(off.astype(np.int64)))
    assert got.is_cuda and (host(got) == want).all()
    assert (hash_to.sha256_to_fr(eng, [b"abc", b""]) == tc.sha_expected([b"abc", b""], True)).all()
