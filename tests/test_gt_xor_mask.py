"""The XOR mask from GT bytes (csrc/mask29.hip.hpp, the entries in csrc/gpbc_wire.hip, include/gpbc_bn254_mask.h), CPU part: the case
list of mask_cases.py covers what it claims, the new header against _lib.MASK_SIGNATURES, the build's dependency lists, and the
argument checks of the C entries and of bn254.gt_xor_mask, which need no device.  The kernel itself runs in test_gt_xor_mask_gpu.py."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
import abi_headers
import mask_cases as mc

VP = ctypes.c_void_p
INVALID_ARG = -1


# ------------------------------------------------------------------------------------------------ the case list
def test_case_list_covers_what_it_claims():
    cases = mc.cases()
    assert [c["label"] for c in cases] == mc.case_ids()
    assert sorted(mc.ORDER) == mc.LENGTHS == [0, 1, 31, 32, 33, 63, 64, 65, 383, 384, 385, 500]
    assert mc.ORDER[0] == 1 and 0 < mc.ORDER.index(0) < len(mc.ORDER) - 1                 # a 1-byte message first, the empty one in the middle
    assert mc.KIND_NAMES == ["zero", "one", "pairing", "p-1", "first-zero"]
    masks = {name: mask for name, _, mask in mc.KINDS}
    assert masks["zero"] == bytes(384) and masks["one"] == bytes(383) + b"\x01"
    assert masks["p-1"] == (mc.P - 1).to_bytes(32, "big") * 12
    assert masks["first-zero"][:32] == bytes(32) and any(masks["first-zero"][32:64])
    assert len(set(masks["pairing"][32 * w:32 * w + 32] for w in range(12))) == 12 and all(int.from_bytes(masks["pairing"][32 * w:32 * w + 32], "big") < mc.P for w in range(12))
    for name, row, mask in mc.KINDS:                                                       # in-memory bytes and GT.Bytes() are the same element
        assert row.shape == (384,) and mc.mask_of(row) == mask, name
    ragged = {c["n"]: c for c in cases if c["width"] is None}
    assert sorted(ragged) == [1, 21, 22, 65] and 21 * 12 < 256 < 22 * 12 and 65 > 64
    big = ragged[65]
    assert {(len(m), k) for m, k in zip(big["msgs"], big["kinds"])} == {(L, k) for L in mc.LENGTHS for k in range(5)}
    for c in ragged.values():
        off = c["off"]
        assert int(off[0]) == mc.LEAD and c["data"].size == int(off[-1]) + mc.TRAIL and (c["data"][:mc.LEAD] != 0).all() and (c["data"][int(off[-1]):] != 0).all()
        assert [int(b - a) for a, b in zip(off[:-1], off[1:])] == [len(m) for m in c["msgs"]]
        assert (c["want"][:mc.LEAD] == c["data"][:mc.LEAD]).all() and (c["want"][int(off[-1]):] == c["data"][int(off[-1]):]).all()
    whole = [int(s) for s, m in zip(ragged[65]["off"][:-1], ragged[65]["msgs"]) if len(m) >= 32]      # items with a whole piece, by address path
    assert any(s % 16 == 0 for s in whole) and any(s % 16 and s % 4 == 0 for s in whole) and any(s % 2 for s in whole)
    assert int(ragged[65]["off"][1]) % 2 == 0 and int(ragged[65]["off"][0]) % 2 == 1
    rows = {c["width"]: c for c in cases if c["width"] is not None}
    assert sorted(rows) == [1, 32, 33, 384, 400] and all(c["n"] == mc.ROWS == 300 and len(set(c["kinds"])) == 5 for c in rows.values())      # 300 x 1 lane crosses a workgroup too
    for c in cases:
        assert c["want_len"].tolist() == [min(len(m), 384) for m in c["msgs"]]


def test_expectation_is_xor_cut_to_the_shorter_operand():
    """the reference's utils.Xor: the shorter length, then (here) zeros to the message's end"""
    mask = bytes(range(1, 256)) + bytes(129)
    assert mc.xor_cut(b"", mask) == (b"", 0)
    assert mc.xor_cut(b"\xff\x00", mask) == (b"\xfe\x02", 2)
    out, L = mc.xor_cut(b"\xaa" * 500, mask)
    assert L == 384 and out[:384] == bytes(0xAA ^ b for b in mask) and out[384:] == bytes(116)


# ------------------------------------------------------------------------------------------------ the header, the tables, the build
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


def test_mask_signature_table_is_the_mask_header(lib):
    from gopairingbasedcryptography_amd import _lib
    protos = abi_headers.prototypes("gpbc_bn254_mask.h")
    assert sorted(protos) == sorted(_lib.MASK_SIGNATURES) == ["gpbc_gt_xor_mask", "gpbc_gt_xor_mask_dev", "gpbc_mask_version"]
    ctype = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int}
    for name, (ret, params) in protos.items():
        assert _lib.MASK_SIGNATURES[name] == ret + ":" + "".join(params), name
        fn = getattr(lib, name)                                                            # load() declared it
        assert fn.restype is ctype[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [ctype[k] for k in params], name
    assert lib.gpbc_mask_version() == 1 and lib.gpbc_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "gpbc_bn254_mask.h")).read()
    assert '#include "gpbc_bn254.h"' in header
    assert all(cite in header for cite in ("bf01_ibe.go:170-176", ":202-208", "hash_from_gt.go:5-8", "xor.go:3-16"))


def test_build_lists_cover_the_new_header_and_no_new_unit():
    from gopairingbasedcryptography_amd import _build
    assert "mask29.hip.hpp" in _build.HEADERS and os.path.exists(os.path.join(_build.CSRC, "mask29.hip.hpp"))
    assert not os.path.exists(os.path.join(_build.CSRC, "gpbc_mask.hip")) and "gpbc_mask.hip" not in _build.UNITS
    unit = open(os.path.join(_build.CSRC, "gpbc_wire.hip")).read()
    assert '#include "mask29.hip.hpp"' in unit and "k_gt_xor_mask" in unit and "gpbc_bn254_mask.h" in unit


# ------------------------------------------------------------------------------------------------ the C entries
def test_c_entries_reject_invalid_arguments(lib):
    """GPBC_ERR_INVALID_ARG with a message, nothing written, before any device is touched; n == 0 is a no-op whatever the pointers"""
    p = lambda a: VP(a.ctypes.data)
    gt, msgs, out = np.zeros(2 * 384, np.uint8), np.zeros(8, np.uint8), np.full(8, 0xA5, np.uint8)
    out_len = np.full(2, 0xA5A5A5A5, np.uint32)
    off, down, empty = np.array([0, 3, 8], dtype=np.uint64), np.array([0, 5, 3], dtype=np.uint64), np.array([4, 4, 4], dtype=np.uint64)
    H, D = lib.gpbc_gt_xor_mask, lib.gpbc_gt_xor_mask_dev
    both = np.zeros(2 * 384 + 8, np.uint8)
    bad = [
        lambda: H(None, p(msgs), p(off), 0, 2, p(out), p(out_len)),                        # null gt
        lambda: H(p(gt), None, p(off), 0, 2, p(out), p(out_len)),                          # null msgs / out where a message has a byte
        lambda: H(p(gt), p(msgs), p(off), 0, 2, None, p(out_len)),
        lambda: H(p(gt), None, None, 4, 2, p(out), None),                                  # ... in row mode
        lambda: H(p(gt), p(msgs), None, 4, 2, None, None),
        lambda: H(None, None, None, 0, 2, None, None),                                     # width 0 still needs gt
        lambda: H(p(gt), p(msgs), p(down), 0, 2, p(out), p(out_len)),                      # decreasing offsets
        lambda: H(p(gt), p(msgs), None, 4, 2, VP(msgs.ctypes.data + 2), None),             # out overlaps msgs without being msgs
        lambda: H(p(both), VP(both.ctypes.data + 768), None, 4, 2, VP(both.ctypes.data + 766), None),      # out overlaps gt
        lambda: H(p(gt), p(msgs), None, 1 << 63, 2, p(out), None),                         # n * width overflows
        lambda: D(None, p(msgs), p(off), 8, 0, 2, p(out), p(out_len), None),
        lambda: D(p(gt), None, p(off), 8, 0, 2, p(out), p(out_len), None),
        lambda: D(p(gt), p(msgs), p(off), 8, 0, 2, None, p(out_len), None),
        lambda: D(p(gt), p(msgs), None, 7, 4, 2, p(out), None, None),                      # row mode: n * width > msgs_bytes
        lambda: D(p(gt), None, None, 8, 4, 2, p(out), None, None),
        lambda: D(p(both), VP(both.ctypes.data + 768), None, 8, 4, 2, VP(both.ctypes.data + 766), None, None),
    ]
    for i, call in enumerate(bad):
        assert call() == INVALID_ARG and lib.gpbc_last_error(), i
    assert b"decrease" in (H(p(gt), p(msgs), p(down), 0, 2, p(out), p(out_len)), lib.gpbc_last_error())[1]
    assert b"overlaps gt" in (H(p(both), VP(both.ctypes.data + 768), None, 4, 2, VP(both.ctypes.data + 766), None), lib.gpbc_last_error())[1]
    assert (out == 0xA5).all() and (out_len == 0xA5A5A5A5).all() and not msgs.any()
    assert H(None, None, None, 0, 0, None, None) == 0 and D(None, None, None, 0, 0, 0, None, None, None) == 0
    assert H(None, None, p(down), 9, 0, None, None) == 0                                   # n == 0: nothing is looked at


def test_wrapper_rejects_malformed_arguments():
    """ValueError before any C call (no device is touched: this runs without a GPU)"""
    import torch
    from gopairingbasedcryptography_amd import bn254
    z = lambda *s: np.zeros(s, dtype=np.uint8)
    t = lambda *s: torch.zeros(s, dtype=torch.uint8)
    slots = bn254._slots
    M = bn254.gt_xor_mask
    off = np.array([0, 3, 8], dtype=np.uint64)
    bad = [
        lambda: M(z(3, 384), [b"a", b"b"]),                                                # three GT rows, two messages
        lambda: M(z(2, 384), z(8), off[:2]),
        lambda: M(z(1, 384), z(2, 16)),
        lambda: M(z(2, 383), z(2, 16)),                                                    # not whole rows
        lambda: M(t(2, 384), [b"a", b"b"]),                                                # GT on one side, messages on the other
        lambda: M(t(2, 384), z(2, 16)),
        lambda: M(z(2, 384), t(2, 16)),
        lambda: M(z(2, 384), t(8), torch.tensor([0, 3, 8])),
        lambda: M(t(2, 384), t(8), torch.tensor([0, 3, 8], dtype=torch.int32)),            # a device msg_off of the wrong dtype
        lambda: M(t(2, 384), t(8), off),
        lambda: M(t(2, 384), t(8)),                                                        # a flat tensor needs offsets
        lambda: M(z(2, 384), z(8)),                                                        # ... and so does a flat array
        lambda: M(z(2, 384), b"abcdefgh"),
        lambda: M(t(2, 384), t(2, 16)),                                                    # one kind, but host tensors: not CUDA
        lambda: M(t(2, 384), t(8), torch.tensor([0, 3, 8])),
        lambda: M(z(2, 384), z(8), np.array([0, 4, 9], dtype=np.uint64)),                  # offsets past the buffer
        lambda: M(z(2, 384), z(2, 16), out=z(2, 15)),                                      # wrong out
        lambda: M(z(2, 384), z(2, 16), out=t(2, 16)),
        lambda: M(z(2, 384), z(8), off, out=z(9)),
        lambda: M(z(2, 384), z(2, 16), out=z(2, 32)[:, :16]),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d was accepted" % i)
        assert bn254._slots is slots, i
    buf = z(40)
    with pytest.raises(ValueError, match="overlaps"):                                      # out overlaps the messages without being them
        M(z(2, 384), buf[:32].reshape(2, 16), out=buf[8:].reshape(2, 16))
    assert bn254._slots is slots
    out, out_len = M(z(0, 384), z(0, 16))                                                  # nothing to do: no engine call
    assert out.shape == (0, 16) and out_len.shape == (0,) and out_len.dtype == np.uint32 and bn254._slots is slots
    (flat, offsets), out_len = M(z(0, 384), [])
    assert flat.shape == (0,) and offsets.tolist() == [0] and out_len.shape == (0,) and bn254._slots is slots


def test_no_cpu_fallback_for_the_mask(lib):
    """without a GPU a well-formed call returns a negative status and leaves a message; nothing is written"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gopairingbasedcryptography_amd import bn254, EngineError
    case = mc.cases()[1]
    with pytest.raises(EngineError):
        bn254.gt_xor_mask(case["gt"], case["msgs"])
    with pytest.raises(EngineError):
        bn254.gt_xor_mask(case["gt"], case["data"].copy(), case["off"])
    rows, _ = mc.rows_of(mc.cases()[5])
    with pytest.raises(EngineError):
        bn254.gt_xor_mask(mc.cases()[5]["gt"], rows.copy())
    gt, msgs, out = case["gt"][:1].copy(), np.zeros(32, np.uint8), np.full(32, 0xA5, np.uint8)
    assert lib.gpbc_gt_xor_mask(VP(gt.ctypes.data), VP(msgs.ctypes.data), None, 32, 1, VP(out.ctypes.data), None) < 0 and lib.gpbc_last_error()
    assert (out == 0xA5).all()
