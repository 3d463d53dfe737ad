"""The oracle of the seed-addressed generator (include/gpbc_bn254_random.h): the ChaCha20 block function of RFC 8439 section 2.3 and
scalar() = OS2IP(block) mod r in plain Python integers, written from the RFC and held against tests/golden/chacha20_blocks.json (openssl's
blocks, one invocation each) by tests/test_random_bounds.py.  Shared by the CPU and the GPU tests; nothing here touches the package."""
import functools
import json
import os
import struct

import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
M32, M64 = 0xFFFFFFFF, (1 << 64) - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chacha20_blocks.json")
RFC_SEED = bytes(range(32))
RFC_INDEX, RFC_STREAM = 0x0900000000000001, 0x4A000000
SEED_B = bytes((i * 73 + 41) % 256 for i in range(32))


def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & M32


def _quarter(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 7)


def block(seed, stream, index):
    """the 64 bytes of block `index` of `stream` under the 32-byte `seed`"""
    assert len(seed) == 32 and 0 <= stream <= M64 and 0 <= index <= M64
    state = list(struct.unpack("<4I", b"expand 32-byte k")) + list(struct.unpack("<8I", seed)) + [index & M32, index >> 32, stream & M32, stream >> 32]
    x = list(state)
    for _ in range(10):
        _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
        _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
    return struct.pack("<16I", *[(a + b) & M32 for a, b in zip(x, state)])


def reduce64(b):
    """OS2IP of a 64-byte string, mod r"""
    assert len(b) == 64
    return int.from_bytes(b, "big") % R


def scalar(seed, stream, index):
    return reduce64(block(seed, stream, index))


def blocks(seed, stream, first, n):
    """[n, 64] uint8: blocks first .. first + n - 1 (first + n <= 2^64)"""
    assert first + n <= 1 << 64
    return np.frombuffer(b"".join(block(seed, stream, first + i) for i in range(n)), dtype=np.uint8).reshape(n, 64).copy()


def scalars(seed, stream, first, n):
    """[n, 32] uint8: the scalars first .. first + n - 1 in the ABI's scalar format"""
    assert first + n <= 1 << 64
    return np.frombuffer(b"".join(scalar(seed, stream, first + i).to_bytes(32, "little") for i in range(n)), dtype=np.uint8).reshape(n, 32).copy()


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# the strings the reduction is held against: the extremes of both halves, then 256 seeded random strings
def _pair(hi, lo):
    return hi.to_bytes(32, "big") + lo.to_bytes(32, "big")


TOP = (1 << 256) - 1
EXTREME = [_pair(0, 0), _pair(TOP, TOP)] + [_pair(0, lo) for lo in (R - 1, R, R + 1, TOP)] + [_pair(hi, 0) for hi in (1, R - 1, R, TOP)]


@functools.lru_cache(maxsize=None)
def reduce_strings():
    rng = np.random.RandomState(20261020)
    return EXTREME + [rng.bytes(64) for _ in range(256)]


def strings_array(strings):
    return np.frombuffer(b"".join(strings), dtype=np.uint8).reshape(len(strings), 64)


def reduced_array(strings):
    return np.frombuffer(b"".join(reduce64(s).to_bytes(32, "little") for s in strings), dtype=np.uint8).reshape(len(strings), 32)
