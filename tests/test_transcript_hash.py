"""The transcript hash H(u, v, w) and the plain SHA-256 (csrc/transcript29.hip.hpp, csrc/gpbc_hash.hip, include/gpbc_bn254_hash.h), CPU part.

hc_hash_g1_gt_gt_to_fr and hc_sha256 (tools/bounds_check.cpp) are the lane functions of the two kernels compiled for the host with
-DGPBC_BOUNDS — every product of the 25 coordinate conversions and of the final reduction asserts its int64 columns — held against
hashlib over the oracle's encodings on the case lists of transcript_cases.py.  Then the new header against _lib.HASH_SIGNATURES, the
wrappers' and the C entries' argument checks, which need no device, and the two thin Python callers on a hashlib stand-in."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from conftest import ROOT
from bounds_harness import hc  # noqa: F401  (the fixture)
import abi_headers
import transcript_cases as tc

VP = ctypes.c_void_p


def hc_sha(hc, msgs, to_fr, total=None):
    data, off = tc.flat_messages(msgs)
    out = np.full((len(msgs), 32), 0xA5, dtype=np.uint8)
    hc.hc_sha256(data.ctypes.data, off.ctypes.data, int(off[-1]) if total is None else total, len(msgs), to_fr, out.ctypes.data)
    return out


# ------------------------------------------------------------------------------------------------ the lane functions
def test_case_list_reaches_the_edges(oracle):
    """the expected streams themselves: all four first-byte forms occur, and the seeded walk for a leading zero byte"""
    names, u, v, w, _ = tc.transcript_arrays(oracle)
    items = tc.transcript_items(oracle)
    first = {n.split("/")[0]: tc.o.g1_marshal(pt, compressed=True) for n, pt, _, _ in items if "/" in n}
    assert first["inf"] == bytes([0x40]) + bytes(31) and not u[names.index("inf/zero/zero")].any()
    assert first["gen"][0] & 0xC0 == 0x80 and {first["5g"][0] & 0xC0, first["-5g"][0] & 0xC0} == {0x80, 0xC0} and first["5g"][1:] == first["-5g"][1:]
    if tc.leading_zero_point() is None:
        pytest.skip("no [k] g1 with X < 2^248 within 2^12 steps of the seeded walk")
    assert first["x<2^248"][0] in (0x80, 0xC0)
    assert len(items) == 5 * 16 + 32


def test_transcript_under_bounds(hc, oracle):
    """every item against hashlib over the oracle's encodings, bit for bit; a finished run is the overflow proof"""
    names, u, v, w, want = tc.transcript_arrays(oracle)
    got = np.full_like(want, 0xA5)
    hc.hc_hash_g1_gt_gt_to_fr(u.ctypes.data, v.ctypes.data, w.ctypes.data, len(names), got.ctypes.data)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), [names[i] for i in bad[:8]]
    assert all(int.from_bytes(r.tobytes(), "little") < tc.R for r in got)


@pytest.mark.parametrize("to_fr", [0, 1])
def test_sha256_under_bounds(hc, to_fr):
    msgs = tc.sha_messages()
    got = hc_sha(hc, msgs, to_fr)
    want = tc.sha_expected(msgs, to_fr)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), [len(msgs[i]) for i in bad]
    if not to_fr:
        for (m, hexdigest), row in zip(tc.KNOWN, got[len(tc.SHA_LENGTHS):]):
            assert row.tobytes().hex() == hexdigest, m


def test_sha256_offsets_are_clamped(hc):
    """offsets past the buffer act as its end (msg_range): the last message is cut, the ones behind it are empty"""
    msgs = [b"0123456789" * 7, b"abc", b"tail"]
    got = hc_sha(hc, msgs, 0, total=72)
    assert (got == tc.sha_expected([msgs[0], b"ab", b""], 0)).all()


def test_digest_above_r_is_reduced(hc):
    """a digest at or above r (about four in five are): to_fr is not the digest's bytes reversed"""
    msgs = tc.sha_messages()
    digests = [int.from_bytes(hashlib.sha256(m).digest(), "big") for m in msgs]
    assert any(d >= tc.R for d in digests) and any(d >= 4 * tc.R for d in digests)


# ------------------------------------------------------------------------------------------------ the header, the wrappers, the C entries
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


def test_hash_signature_table_is_the_hash_header(lib):
    from gopairingbasedcryptography_amd import _lib
    protos = abi_headers.prototypes("gpbc_bn254_hash.h")
    assert sorted(protos) == sorted(_lib.HASH_SIGNATURES) and len(protos) == 5
    ctype = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int}
    for name, (ret, params) in protos.items():
        assert _lib.HASH_SIGNATURES[name] == ret + ":" + "".join(params), name
        fn = getattr(lib, name)
        assert fn.restype is ctype[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [ctype[k] for k in params], name
    assert lib.gpbc_hash_version() == 1 and lib.gpbc_abi_version() == 8
    assert '#include "gpbc_bn254.h"' in open(os.path.join(ROOT, "include", "gpbc_bn254_hash.h")).read()


def test_source_hash_covers_the_new_header_and_unit():
    from gopairingbasedcryptography_amd import _build
    assert "gpbc_hash.hip" in _build.UNITS and "transcript29.hip.hpp" in _build.HEADERS


def test_wrappers_reject_malformed_arguments():
    """ValueError before any C call (no device is touched: this runs without a GPU)"""
    import torch
    from gopairingbasedcryptography_amd import bn254
    z = lambda *s: np.zeros(s, dtype=np.uint8)
    t = lambda *s: torch.zeros(s, dtype=torch.uint8)
    slots = bn254._slots
    H, S = bn254.hash_g1_gt_gt_to_fr, bn254.sha256
    bad = [
        lambda: H(z(2, 64), z(2, 384), t(2, 384)),                                   # mixed kinds
        lambda: H(t(2, 64), z(2, 384), z(2, 384)),
        lambda: H(z(2, 64), z(2, 384), z(2, 384), out=t(2, 32)),
        lambda: H(t(2, 64), t(2, 384), t(2, 384)),                                   # one kind, but host tensors: not CUDA
        lambda: H(z(2, 64), z(1, 384), z(2, 384)),                                   # row counts differ
        lambda: H(z(2, 64), z(2, 384), z(3, 384)),
        lambda: H(z(65), z(384), z(384)),                                            # not whole rows
        lambda: H(z(2, 64), z(2, 383), z(2, 384)),
        lambda: H(z(2, 64), z(2, 384), z(2, 384), out=z(2, 31)),                     # wrong out
        lambda: H(z(2, 64), z(2, 384), z(2, 384), out=np.zeros((2, 32), dtype=np.int8)),
        lambda: H(z(2, 64), z(2, 384), z(2, 384), out=z(2, 64)[:, :32]),
        lambda: S(t(8)),                                                             # a tensor needs offsets
        lambda: S(t(8), torch.zeros(3, dtype=torch.int32)),
        lambda: S(t(8), np.zeros(3, dtype=np.uint64)),
        lambda: S(t(8), torch.zeros(3, dtype=torch.int64)),                          # host tensors
        lambda: S(z(8), np.array([0, 4, 9], dtype=np.uint64)),                       # offsets past the buffer
        lambda: S([b"a", b"b"], out=z(3, 32)),
        lambda: S([b"a", b"b"], out=t(2, 32)),
        lambda: S([b"a", b"b"], to_fr=True, out=z(2, 32)[::-1]),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d was accepted" % i)
        assert bn254._slots is slots, i
    assert S([]).shape == (0, 32) and bn254._slots is slots                          # nothing to hash: no engine call


def test_c_entries_reject_invalid_arguments(lib):
    """GPBC_ERR_INVALID_ARG with a message, nothing written, before any device is touched; n == 0 is a no-op whatever the pointers"""
    p = lambda a: VP(a.ctypes.data)
    u, v, w, out = np.zeros(2 * 64, np.uint8), np.zeros(2 * 384, np.uint8), np.zeros(2 * 384, np.uint8), np.full(2 * 32, 0xA5, np.uint8)
    msgs, off = np.zeros(8, np.uint8), np.array([0, 3, 8], dtype=np.uint64)
    down = np.array([0, 5, 3], dtype=np.uint64)
    bad = [lambda: lib.gpbc_hash_g1_gt_gt_to_fr(None, p(v), p(w), 2, p(out)), lambda: lib.gpbc_hash_g1_gt_gt_to_fr(p(u), None, p(w), 2, p(out)),
           lambda: lib.gpbc_hash_g1_gt_gt_to_fr(p(u), p(v), None, 2, p(out)), lambda: lib.gpbc_hash_g1_gt_gt_to_fr(p(u), p(v), p(w), 2, None),
           lambda: lib.gpbc_hash_g1_gt_gt_to_fr_dev(None, p(v), p(w), 2, p(out), None), lambda: lib.gpbc_hash_g1_gt_gt_to_fr_dev(p(u), p(v), p(w), 2, None, None),
           lambda: lib.gpbc_sha256_batch(p(msgs), None, 2, 0, p(out)), lambda: lib.gpbc_sha256_batch(p(msgs), p(off), 2, 1, None),
           lambda: lib.gpbc_sha256_batch(None, p(off), 2, 0, p(out)), lambda: lib.gpbc_sha256_batch(p(msgs), p(down), 2, 0, p(out)),
           lambda: lib.gpbc_sha256_batch_dev(p(msgs), None, 8, 2, 0, p(out), None), lambda: lib.gpbc_sha256_batch_dev(p(msgs), p(off), 8, 2, 0, None, None),
           lambda: lib.gpbc_sha256_batch_dev(None, p(off), 8, 2, 0, p(out), None)]
    for i, call in enumerate(bad):
        assert call() == -1 and lib.gpbc_last_error(), i
    assert b"decrease" in (lib.gpbc_sha256_batch(p(msgs), p(down), 2, 0, p(out)), lib.gpbc_last_error())[1]
    assert (out == 0xA5).all()
    assert lib.gpbc_hash_g1_gt_gt_to_fr(None, None, None, 0, None) == 0 and lib.gpbc_hash_g1_gt_gt_to_fr_dev(None, None, None, 0, None, None) == 0
    assert lib.gpbc_sha256_batch(None, None, 0, 0, None) == 0 and lib.gpbc_sha256_batch_dev(None, None, 0, 0, 1, None, None) == 0


def test_no_cpu_fallback_for_the_hashes(lib, oracle):
    """without a GPU a well-formed call returns a negative status and leaves a message"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gopairingbasedcryptography_amd import bn254, EngineError
    _, u, v, w, _ = tc.transcript_arrays(oracle)
    with pytest.raises(EngineError):
        bn254.hash_g1_gt_gt_to_fr(u[:2], v[:2], w[:2])
    with pytest.raises(EngineError):
        bn254.sha256([b"abc"])
    out = np.full(32, 0xA5, np.uint8)
    assert lib.gpbc_hash_g1_gt_gt_to_fr(VP(u.ctypes.data), VP(v.ctypes.data), VP(w.ctypes.data), 1, VP(out.ctypes.data)) < 0 and lib.gpbc_last_error()
    assert (out == 0xA5).all()


# ------------------------------------------------------------------------------------------------ the thin callers
class HashlibEngine:
    """bn254.sha256 on hashlib, recording how it was called"""

    def __init__(self):
        self.calls = []

    def sha256(self, msgs, msg_off=None, to_fr=False, out=None):
        self.calls.append((msg_off is not None, to_fr))
        if msg_off is not None:
            buf = np.asarray(msgs, dtype=np.uint8).tobytes()
            msgs = [buf[int(a):int(b)] for a, b in zip(msg_off[:-1], msg_off[1:])]
        return tc.sha_expected([bytes(m) for m in msgs], to_fr)


def test_thin_callers_pass_through():
    from gopairingbasedcryptography_amd import hash_to, waters05
    eng = HashlibEngine()
    names = ["alice@example.com", b"bob", "carol"]
    assert (waters05.identity_masks_device(eng, names) == waters05.identity_masks(names)).all()
    data, off = tc.flat_messages([n.encode() if isinstance(n, str) else n for n in names])
    assert (waters05.identity_masks_device(eng, data, off) == waters05.identity_masks(names)).all()
    with pytest.raises(ValueError):
        waters05.identity_masks_device(eng, ["alice", ""])
    msgs = tc.sha_messages()
    assert (hash_to.sha256_to_fr(eng, msgs) == tc.sha_expected(msgs, 1)).all()
    assert eng.calls == [(False, False), (True, False), (False, True)]
    assert "sha256_to_fr" in hash_to.__doc__ and "hash_g1_gt_gt_to_fr" in hash_to.__doc__
