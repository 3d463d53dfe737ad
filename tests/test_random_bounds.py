"""The seed-addressed generator on the CPU: the oracle of tests/chacha_cases.py against openssl's blocks (tests/golden/chacha20_blocks.json),
then the device header csrc/chacha29.hip.hpp and fr_wide_reduce of csrc/fr29.hip.hpp compiled for the host with -DGPBC_BOUNDS
(tools/bounds_check.cpp: hc_chacha_blocks, hc_fr_wide_reduce, hc_fr_random) against that oracle, exactly.  Under GPBC_BOUNDS every product
asserts its int64 columns and fr_canonical its input range, and a violation aborts: a run that finishes is the overflow proof."""

import numpy as np

from bounds_harness import hc  # noqa: F401  (the fixture)
import chacha_cases as cc

GUARD = 0xA5


def aligned(n, shift=0):
    """n guard bytes starting `shift` bytes behind a 16-byte boundary"""
    raw = np.full(n + 32, GUARD, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16 + shift
    return raw[off:off + n]


def seed_buf(seed):
    return np.frombuffer(seed, dtype=np.uint8).copy()


# ------------------------------------------------------------------------------------------------ the oracle against openssl
def test_fixture_holds_what_it_claims():
    g = cc.golden()
    assert "openssl enc -chacha20" in g["command"] and g["openssl"].startswith("OpenSSL")
    rows = g["blocks"]
    rfc = rows[0]
    assert (bytes.fromhex(rfc["seed"]), rfc["index"], rfc["stream"]) == (cc.RFC_SEED, cc.RFC_INDEX, cc.RFC_STREAM)
    assert rfc["block"].startswith("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e") and rfc["block"].endswith("a2503c4e")
    assert {bytes.fromhex(r["seed"]) for r in rows} == {cc.RFC_SEED, cc.SEED_B}
    for seed in (cc.RFC_SEED, cc.SEED_B):
        have = {(r["index"], r["stream"]) for r in rows if bytes.fromhex(r["seed"]) == seed}
        assert have >= {(i, s) for i in (0, 1, 2**32 - 1, 2**32, 2**64 - 1) for s in (0, 0x4A000000, 2**64 - 1)}
    assert len({r["block"] for r in rows}) == len(rows) == 31 and all(len(r["block"]) == 128 for r in rows)


def test_python_block_is_openssls():
    for r in cc.golden()["blocks"]:
        assert cc.block(bytes.fromhex(r["seed"]), r["stream"], r["index"]).hex() == r["block"], r


def test_python_scalar_is_the_big_endian_integer_mod_r():
    b = cc.block(cc.RFC_SEED, cc.RFC_STREAM, cc.RFC_INDEX)
    assert b[0] == 0x10 and cc.scalar(cc.RFC_SEED, cc.RFC_STREAM, cc.RFC_INDEX) == sum(v << 8 * (63 - i) for i, v in enumerate(b)) % cc.R
    assert [cc.reduce64(s) for s in cc.EXTREME[:3]] == [0, ((1 << 512) - 1) % cc.R, cc.R - 1]
    assert cc.scalars(cc.SEED_B, 3, 5, 2)[1].tobytes() == cc.scalar(cc.SEED_B, 3, 6).to_bytes(32, "little")
    assert len(cc.reduce_strings()) == 10 + 256 and len(set(cc.reduce_strings())) == 266


# ------------------------------------------------------------------------------------------------ the device header on the host
def test_hc_chacha_blocks_equals_the_fixture(hc):
    for r in cc.golden()["blocks"]:
        seed = seed_buf(bytes.fromhex(r["seed"]))
        for wide, shift in ((1, 0), (0, 3)):
            out = aligned(64 + 16, shift)
            assert hc.hc_chacha_blocks(seed.ctypes.data, r["stream"], r["index"], 1, out.ctypes.data, wide) == 0
            assert out[:64].tobytes().hex() == r["block"] and (out[64:] == GUARD).all(), (r, wide)


def test_hc_chacha_blocks_carries_into_the_high_word(hc):
    """a run of indices across 2^32 is the oracle's, block by block; first + n may reach 2^64 and not pass it"""
    seed = seed_buf(cc.SEED_B)
    for first, n in ((2**32 - 3, 6), (2**64 - 5, 5), (0, 3)):
        out = aligned(64 * n + 16)
        assert hc.hc_chacha_blocks(seed.ctypes.data, 7, first, n, out.ctypes.data, 1) == 0
        assert out[:64 * n].tobytes() == cc.blocks(cc.SEED_B, 7, first, n).tobytes() and (out[64 * n:] == GUARD).all()
    out = aligned(64 * 6)
    assert hc.hc_chacha_blocks(seed.ctypes.data, 7, 2**64 - 5, 6, out.ctypes.data, 1) == -1 and (out == GUARD).all()
    assert hc.hc_chacha_blocks(None, 7, 0, 1, out.ctypes.data, 1) == -1 and hc.hc_chacha_blocks(seed.ctypes.data, 7, 0, 1, None, 1) == -1


def test_hc_fr_wide_reduce_equals_python_integers(hc):
    """0, 2^512 - 1, hi = 0 with lo in {r - 1, r, r + 1, 2^256 - 1}, lo = 0 with hi in {1, r - 1, r, 2^256 - 1}, 256 random strings:
    through the 128-bit and the byte loads and stores, a guard behind the output"""
    strings = cc.reduce_strings()
    want = cc.reduced_array(strings)
    n = len(strings)
    for wide_in, wide_out, shift in ((1, 1, 0), (0, 0, 5), (1, 0, 0)):
        src = aligned(64 * n, shift if not wide_in else 0)
        src[:] = cc.strings_array(strings).reshape(-1)
        out = aligned(32 * n + 16, shift if not wide_out else 0)
        assert hc.hc_fr_wide_reduce(src.ctypes.data, n, out.ctypes.data, wide_in, wide_out) == 0
        assert out[:32 * n].tobytes() == want.tobytes() and (out[32 * n:] == GUARD).all(), (wide_in, wide_out)
    assert all(int.from_bytes(row.tobytes(), "little") < cc.R for row in want)


def test_hc_fr_random_is_block_then_reduction(hc):
    seed = seed_buf(cc.RFC_SEED)
    for stream, first, n in ((0, 0, 70), (0x4A000000, 2**32 - 3, 6), (2**64 - 1, 2**64 - 4, 4)):
        out = aligned(32 * n + 16, 1)
        assert hc.hc_fr_random(seed.ctypes.data, stream, first, n, out.ctypes.data) == 0
        assert out[:32 * n].tobytes() == cc.scalars(cc.RFC_SEED, stream, first, n).tobytes() and (out[32 * n:] == GUARD).all()
