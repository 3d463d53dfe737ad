"""The seed-addressed generator (include/gpbc_bn254_random.h), the part that needs no device: the new header against
_lib.RANDOM_SIGNATURES, the build's dependency lists, the argument checks of the C entries and of the Python wrappers, rng.Randomness
over a recording engine, and the loud failure of the host entries where there is no GPU."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT
import abi_headers
import chacha_cases as cc
from gopairingbasedcryptography_amd import _build, _lib

HEADER = os.path.join(ROOT, "include", "gpbc_bn254_random.h")
NAMES = ["gpbc_fr_random", "gpbc_fr_random_dev", "gpbc_fr_set_bytes64", "gpbc_fr_set_bytes64_dev", "gpbc_random_bytes", "gpbc_random_bytes_dev", "gpbc_random_version"]
SEED = bytes(range(100, 132))                       # no four of these bytes appear in a message by accident


@pytest.fixture(scope="module")
def lib():
    _build.build_library()
    return _lib.load()


def test_random_signature_table_is_the_random_header(lib):
    protos = abi_headers.prototypes("gpbc_bn254_random.h")
    assert sorted(protos) == sorted(_lib.RANDOM_SIGNATURES) == NAMES
    assert all(set(sig) <= set("pzi:") for sig in _lib.RANDOM_SIGNATURES.values())              # the kinds are p / z / i only
    ctype = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int}
    for name, (ret, params) in protos.items():
        assert _lib.RANDOM_SIGNATURES[name] == ret + ":" + "".join(params), name
        fn = getattr(lib, name)
        assert fn.restype is ctype[ret] and list(fn.argtypes) == [ctype[k] for k in params], name
    assert lib.gpbc_random_version() == 1 and lib.gpbc_formula_version() == 1 and lib.gpbc_hash_version() == 1 and lib.gpbc_abi_version() == 8
    assert ctypes.sizeof(ctypes.c_size_t) == 8                                                    # LP64: stream and first are 64-bit
    header = open(HEADER).read()
    assert '#include "gpbc_bn254.h"' in header and "Entry map" in header and "0x0900000000000001" in header and "KEY MATERIAL" in header


def test_build_lists_cover_the_new_header_and_lane_functions():
    assert "chacha29.hip.hpp" in _build.HEADERS and not os.path.exists(os.path.join(_build.CSRC, "gpbc_random.hip"))
    unit = open(os.path.join(_build.CSRC, "gpbc_hash.hip")).read()
    assert 'include "chacha29.hip.hpp"' in unit and 'gpbc_bn254_random.h"' in unit
    assert all(k in unit for k in ("k_random_bytes", "k_fr_random", "k_fr_set_bytes64", "fr_wide_reduce("))
    lane = open(os.path.join(_build.CSRC, "chacha29.hip.hpp")).read()
    assert "asm" not in lane and "__builtin_rotateleft32" in lane and "chacha20_block(" in lane
    assert "fr_wide_reduce(" in open(os.path.join(_build.CSRC, "fr29.hip.hpp")).read()
    harness = open(os.path.join(ROOT, "tools", "bounds_check.cpp")).read()
    assert all(name + "(" in harness for name in ("hc_chacha_blocks", "hc_fr_wide_reduce", "chacha20_block", "fr_wide_reduce"))


# ------------------------------------------------------------------------------------------------ arguments, without a device
def test_c_entries_reject_invalid_arguments(lib):
    """GPBC_ERR_INVALID_ARG with a message that shows no seed byte, nothing written, before any device is touched; a count of 0 is a
    no-op whatever the pointers"""
    seed = (ctypes.c_char * 32).from_buffer_copy(SEED)
    out = np.zeros(4096, np.uint8)
    O, TOP = out.ctypes.data, (1 << 64) - 1
    for name in ("gpbc_random_bytes", "gpbc_fr_random"):
        for fn, extra in ((getattr(lib, name), []), (getattr(lib, name + "_dev"), [None])):
            good = [seed, 5, 0, 4, O]
            bad = [(0, None, b"null"), (4, None, b"null"), (2, TOP - 2, b"exceeds 2^64"), (2, TOP, b"exceeds 2^64"), (3, TOP, b"too many"), (3, 1 << 40, b"too many")]
            for at, v, why in bad:
                args = list(good)
                args[at] = v
                assert fn(*args, *extra) == -1, (name, at, v)
                err = lib.gpbc_last_error()
                assert why in err and not any(SEED[i:i + 4] in err for i in range(29)) and SEED.hex()[:8].encode() not in err, (name, at, err)
            edge = [seed, TOP, 1, TOP, O]                                                        # first + n = 2^64 exactly is in range: refused for its size alone
            assert fn(*edge, *extra) == -1 and b"too many" in lib.gpbc_last_error()
            for zero in ([seed, 5, 0, 0, O], [None, 5, TOP, 0, None]):
                assert fn(*zero, *extra) == 0
    src = np.zeros(64 * 8, np.uint8)
    S = src.ctypes.data
    for fn, extra in ((lib.gpbc_fr_set_bytes64, []), (lib.gpbc_fr_set_bytes64_dev, [None])):
        good = [S, 8, O]
        bad = [(0, None, b"null"), (2, None, b"null"), (1, 1 << 40, b"too many"), (2, S, b"overlaps"), (2, S + 511, b"overlaps"), (2, S - 255, b"overlaps"), (0, O + 255, b"overlaps")]
        for at, v, why in bad:
            args = list(good)
            args[at] = v
            assert fn(*args, *extra) == -1 and why in lib.gpbc_last_error(), (at, v, lib.gpbc_last_error())
        for zero in ([S, 0, O], [None, 0, None], [S, 0, S]):
            assert fn(*zero, *extra) == 0
    assert not out.any() and not src.any()


def test_wrappers_reject_malformed_arguments():
    """ValueError before any C call, and never with the seed in the message"""
    import torch
    from gopairingbasedcryptography_amd import bn254
    z = lambda n: np.zeros(n, dtype=np.uint8)
    buf = z(4096)
    bad = [
        (lambda: bn254.fr_random(SEED[:31], 1), "seed must be 32 bytes"), (lambda: bn254.fr_random(list(SEED), 1), "seed must be 32 bytes"),
        (lambda: bn254.random_bytes("x" * 32, 1), "seed must be 32 bytes"), (lambda: bn254.fr_random(SEED, -1), "n must be"),
        (lambda: bn254.fr_random(SEED, 1.0), "n must be"), (lambda: bn254.fr_random(SEED, True), "n must be"),
        (lambda: bn254.fr_random(SEED, 1, stream=1 << 64), "stream must be"), (lambda: bn254.fr_random(SEED, 1, stream=-1), "stream must be"),
        (lambda: bn254.random_bytes(SEED, 1, first=1 << 64), "first must be"), (lambda: bn254.random_bytes(SEED, 2, first=(1 << 64) - 1), "exceeds 2\\^64"),
        (lambda: bn254.fr_random(SEED, 3, out=z(95)), "out must be"), (lambda: bn254.random_bytes(SEED, 3, out=z(96)), "out must be"),
        (lambda: bn254.fr_random(SEED, 3, out=z(96), like=torch.zeros(1, dtype=torch.uint8, device="meta")), "all be CUDA tensors or all host"),
        (lambda: bn254.fr_set_bytes64(z(65)), "whole number of rows of 64"), (lambda: bn254.fr_set_bytes64(z(128), out=z(63)), "out must be"),
        (lambda: bn254.fr_set_bytes64(buf[:128], out=buf[127:191]), "overlaps"), (lambda: bn254.fr_set_bytes64(buf[64:192], out=buf[1:65]), "overlaps"),
    ]
    for fn, why in bad:
        with pytest.raises(ValueError, match=why) as e:
            fn()
        assert SEED.hex()[:8] not in str(e.value) and repr(SEED)[2:10] not in str(e.value)
    assert bn254.fr_random(SEED, 0).shape == (0, 32) and bn254.random_bytes(SEED, 0, first=(1 << 64) - 1).shape == (0, 64)      # nothing to do: no device asked for
    assert bn254.fr_set_bytes64(z(0)).shape == (0, 32)


def test_no_cpu_fallback_for_the_generator(lib):
    """without a GPU the host entries fail loudly and write nothing; with one they give the oracle's bytes"""
    import torch
    from gopairingbasedcryptography_amd import bn254, EngineError
    if torch.cuda.is_available():
        assert bn254.fr_random(cc.RFC_SEED, 3, stream=2).tobytes() == cc.scalars(cc.RFC_SEED, 2, 0, 3).tobytes()
        assert bn254.random_bytes(cc.RFC_SEED, 1, stream=cc.RFC_STREAM, first=cc.RFC_INDEX).tobytes() == cc.block(cc.RFC_SEED, cc.RFC_STREAM, cc.RFC_INDEX)
        return
    for call in (lambda: bn254.fr_random(SEED, 3), lambda: bn254.random_bytes(SEED, 3), lambda: bn254.fr_set_bytes64(np.zeros(128, np.uint8))):
        with pytest.raises(EngineError) as e:
            call()
        assert SEED.hex()[:8] not in str(e.value)
    seed, out = (ctypes.c_char * 32).from_buffer_copy(SEED), np.full(256, 0xA5, np.uint8)
    for fn in (lib.gpbc_fr_random, lib.gpbc_random_bytes):
        assert fn(seed, 0, 0, 2, out.ctypes.data) < 0 and lib.gpbc_last_error() and (out == 0xA5).all()
    assert lib.gpbc_fr_set_bytes64(np.zeros(128, np.uint8).ctypes.data, 2, out.ctypes.data) < 0 and (out == 0xA5).all()


# ------------------------------------------------------------------------------------------------ rng.Randomness
class Recorder:
    """an engine with fr_random alone: the oracle's scalars, every call written down"""

    def __init__(self):
        self.calls = []

    def fr_random(self, seed, n, stream=0, first=0, out=None, like=None):
        self.calls.append((bytes(seed), n, stream, first))
        return cc.scalars(bytes(seed), stream, first, n)


def test_randomness_takes_the_next_stream_per_draw():
    from gopairingbasedcryptography_amd import rng
    eng, like = Recorder(), np.zeros(1, np.uint8)
    r = rng.Randomness(eng, SEED)
    assert r.next_stream == 0
    a, b = r.scalars(like, 5), r.scalars(like, 2, 3)
    assert a.shape == (5, 32) and b.shape == (2, 3, 32) and r.next_stream == 2
    assert a.tobytes() == cc.scalars(SEED, 0, 0, 5).tobytes() and b.tobytes() == cc.scalars(SEED, 1, 0, 6).tobytes()
    assert b[1, 2].tobytes() == cc.scalar(SEED, 1, 5).to_bytes(32, "little")                     # row-major: entry (i, j) is index i * 3 + j
    for shape in ((0,), (4, 0), (0, 7)):
        assert r.scalars(like, *shape).shape == shape + (32,)                                     # no scalars: no stream id, no engine call
    assert r.next_stream == 2 and eng.calls == [(SEED, 5, 0, 0), (SEED, 6, 1, 0)]
    assert r.scalars(like, np.int64(2)).tobytes() == cc.scalars(SEED, 2, 0, 2).tobytes() and r.next_stream == 3
    for shape in ((), (-1,), (2.0,), (True,)):
        with pytest.raises(ValueError, match="shape"):
            r.scalars(like, *shape)
    assert r.next_stream == 3


def test_randomness_keeps_its_seed_to_itself():
    from gopairingbasedcryptography_amd import rng
    r = rng.Randomness(Recorder(), SEED)
    shown = repr(r) + str(r)
    assert "next_stream=0" in shown and SEED.hex() not in shown and repr(SEED) not in shown and SEED.hex()[:8] not in shown
    for bad in (SEED[:16], list(SEED), "s" * 32, 5):
        with pytest.raises(ValueError, match="seed must be 32 bytes") as e:
            rng.Randomness(Recorder(), bad)
        assert "100" not in str(e.value)
    a, b = Recorder(), Recorder()
    rng.Randomness(a).scalars(np.zeros(1, np.uint8), 1)
    rng.Randomness(b).scalars(np.zeros(1, np.uint8), 1)
    assert len(a.calls[0][0]) == 32 and a.calls[0][0] != b.calls[0][0]                           # seed=None: fresh bytes from the system each time
    src = inspect.getsource(rng)
    assert "from . import _buffers as bufs" in src and "_lib" not in src and "import bn254" not in src                # engine-agnostic: the engine is an argument
