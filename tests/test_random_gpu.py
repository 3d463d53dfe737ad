"""The seed-addressed generator on the MI355X (run with -m gpu): gpbc_random_bytes, gpbc_fr_random and gpbc_fr_set_bytes64, host and
_dev forms, against the Python oracle of tests/chacha_cases.py (itself held against openssl's blocks by test_random_bounds.py), exactly:
sizes around the workgroup, `first` across the low word's carry and at the top of the range, the three streams, the RFC 8439 block
through the public entry, guard rows around out=, windows of a large call, every scalar canonical, and the reduction on the extreme
strings."""
import numpy as np
import pytest

import chacha_cases as cc

pytestmark = pytest.mark.gpu
BLOCK = 64                                                  # the kernels' workgroup size (csrc/gpbc_common.hpp)
SIZES = [1, BLOCK - 1, BLOCK, BLOCK + 1, 1000]
STREAMS = [0, 0x4A000000, 2**64 - 1]
GUARD = 0xA5


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def firsts(n):
    """0; three below 2^32, so that the low word carries inside the launch (from n = 4 on); the top of the range without a wrap"""
    return [0, 2**32 - 3, 2**64 - n]


@pytest.fixture(scope="module")
def want():
    """{(stream, first): [1000, 64] blocks}: the oracle once, shared; every size reads its prefix, scalars reduce the same blocks"""
    table = {}
    for stream in STREAMS:
        for n in SIZES:
            for first in firsts(n):
                if (stream, first) not in table:
                    m = max(s for s in SIZES if first + s <= 2**64)
                    table[stream, first] = cc.blocks(cc.SEED_B, stream, first, m)
    return table


def reduced(blocks):
    return np.frombuffer(b"".join(cc.reduce64(b.tobytes()).to_bytes(32, "little") for b in blocks), dtype=np.uint8).reshape(len(blocks), 32)


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("n", SIZES)
def test_bytes_and_scalars_equal_the_oracle(eng, want, n, tensors):
    """both entries, every first and stream; the _dev form on a side stream"""
    import torch
    side = torch.cuda.Stream() if tensors else None
    like = torch.zeros(1, dtype=torch.uint8, device="cuda") if tensors else None
    torch.cuda.synchronize()
    for stream in STREAMS:
        for first in firsts(n):
            blocks = want[stream, first][:n]
            if tensors:
                with torch.cuda.stream(side):
                    b, s = eng.random_bytes(cc.SEED_B, n, stream=stream, first=first, like=like), eng.fr_random(cc.SEED_B, n, stream=stream, first=first, like=like)
                side.synchronize()
                assert b.is_cuda and s.is_cuda
                b, s = b.cpu().numpy(), s.cpu().numpy()
            else:
                b, s = eng.random_bytes(cc.SEED_B, n, stream=stream, first=first), eng.fr_random(cc.SEED_B, n, stream=stream, first=first)
            assert b.shape == (n, 64) and b.tobytes() == blocks.tobytes(), (stream, first)
            assert s.shape == (n, 32) and s.tobytes() == reduced(blocks).tobytes(), (stream, first)


def test_rfc_8439_block_through_the_public_entry(eng):
    import torch
    rfc = bytes.fromhex(cc.golden()["blocks"][0]["block"])
    assert rfc[:8].hex() == "10f1e7e4d13b5915"
    assert eng.random_bytes(cc.RFC_SEED, 1, stream=0x4A000000, first=0x0900000000000001).tobytes() == rfc
    like = torch.zeros(1, dtype=torch.uint8, device="cuda")
    assert eng.random_bytes(cc.RFC_SEED, 1, stream=0x4A000000, first=0x0900000000000001, like=like).cpu().numpy().tobytes() == rfc
    one = eng.fr_random(cc.RFC_SEED, 1, stream=0x4A000000, first=0x0900000000000001)
    assert eng.fr_to_ints(one) == [int.from_bytes(rfc, "big") % cc.R]


def test_out_is_written_between_unchanged_guards(eng, want):
    """guard rows before and after, on a 16-byte boundary and 5 bytes off it; n = 0 leaves the buffer alone"""
    import torch
    n, stream, first = 65, 0x4A000000, 2**32 - 3
    blocks = want[stream, first][:n]
    for name, width, expect in (("random_bytes", 64, blocks), ("fr_random", 32, reduced(blocks))):
        fn = getattr(eng, name)
        for shift in (0, 5):
            host = np.full((n + 2) * width + 32, GUARD, dtype=np.uint8)
            off = (-host.ctypes.data) % 16 + shift + width
            got = fn(cc.SEED_B, n, stream=stream, first=first, out=host[off:off + n * width])
            assert got.shape == (n, width) and host[off:off + n * width].tobytes() == expect.tobytes()
            assert (host[:off] == GUARD).all() and (host[off + n * width:] == GUARD).all()
            dev = torch.full(((n + 2) * width + 32,), GUARD, dtype=torch.uint8, device="cuda")
            off = (-dev.data_ptr()) % 16 + shift + width
            got = fn(cc.SEED_B, n, stream=stream, first=first, out=dev[off:off + n * width])
            back = dev.cpu().numpy()
            assert got.is_cuda and back[off:off + n * width].tobytes() == expect.tobytes()
            assert (back[:off] == GUARD).all() and (back[off + n * width:] == GUARD).all()
        host = np.full(4 * width, GUARD, dtype=np.uint8)
        assert fn(cc.SEED_B, 0, out=host[:0]).shape == (0, width) and (host == GUARD).all()
        dev = torch.full((4 * width,), GUARD, dtype=torch.uint8, device="cuda")
        assert fn(cc.SEED_B, 0, out=dev[:0]).shape == (0, width) and (dev.cpu().numpy() == GUARD).all()


def test_rows_of_a_large_call_are_a_call_that_starts_there(eng):
    """a scalar's value depends on its index alone: rows [a, a + m) of one call over 2^16 equal a call with first = a; every scalar is below r"""
    big_b, big_s = eng.random_bytes(cc.SEED_B, 1 << 16, stream=9), eng.fr_random(cc.SEED_B, 1 << 16, stream=9)
    for a, m in ((0, 3), (63, 130), (40000, 1000), ((1 << 16) - 5, 5)):
        assert eng.random_bytes(cc.SEED_B, m, stream=9, first=a).tobytes() == big_b[a:a + m].tobytes()
        assert eng.fr_random(cc.SEED_B, m, stream=9, first=a).tobytes() == big_s[a:a + m].tobytes()
    assert big_s[40000:40003].tobytes() == cc.scalars(cc.SEED_B, 9, 40000, 3).tobytes()
    top_first = big_s[:, ::-1].copy()                                                  # most significant byte first: row order is integer order
    r_row = np.frombuffer(cc.R.to_bytes(32, "big"), dtype=np.uint8)
    diff = top_first.astype(np.int16) - r_row.astype(np.int16)
    lead = diff[np.arange(len(diff)), (diff != 0).argmax(1)]
    assert (lead < 0).all()                                                            # below r at the first byte that differs, in every row
    assert len({row.tobytes() for row in big_s}) == 1 << 16 and eng.fr_random(cc.SEED_B, 4, stream=8).tobytes() != big_s[:4].tobytes()


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_set_bytes64_on_the_extreme_strings(eng, tensors):
    """0, 2^512 - 1, the halves at r - 1, r, r + 1, 2^256 - 1 and 256 random strings against Python integers; the _dev form on a side stream"""
    import torch
    strings = cc.reduce_strings()
    x, expect = cc.strings_array(strings), cc.reduced_array(strings)
    if tensors:
        side = torch.cuda.Stream()
        xd = torch.from_numpy(x.copy()).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            got = eng.fr_set_bytes64(xd)
            odd = eng.fr_set_bytes64(torch.cat([torch.zeros(3, dtype=torch.uint8, device="cuda"), xd.reshape(-1)])[3:])       # off the 16-byte boundary
        side.synchronize()
        assert got.is_cuda and odd.cpu().numpy().tobytes() == expect.tobytes()
        got = got.cpu().numpy()
        buf = torch.zeros(64 * 4, dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError, match="overlaps"):
            eng.fr_set_bytes64(buf[:128], out=buf[96:160])
    else:
        got = eng.fr_set_bytes64(x)
        assert eng.fr_set_bytes64(b"".join(strings[:3])).tobytes() == expect[:3].tobytes()
        buf = np.zeros(64 * 4, dtype=np.uint8)
        with pytest.raises(ValueError, match="overlaps"):
            eng.fr_set_bytes64(buf[:128], out=buf[96:160])
    assert got.shape == (len(strings), 32) and got.tobytes() == expect.tobytes()
