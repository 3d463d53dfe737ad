"""The common attributes of a list and a set (csrc/select29.hip.hpp; csrc/gpbc_fr.hip: k_fr_find_common; include/gpbc_bn254_select.h),
CPU part.

The kernel as it is launched — geometry, staging into a checked stand-in for the LDS block, the three phases behind it workgroup by
workgroup — compiled for the host with -DGPBC_BOUNDS (tools/bounds_check.cpp: hc_fr_find_common), against utils/find_common_attributes.go
restated in Python integers on every case of tests/select_cases.py, exactly, with guard rows behind all four outputs.  Then the new header
against _lib.SELECT_SIGNATURES, the build's dependency lists, and the argument checks that need no device."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from bounds_harness import hc  # noqa: F401  (the fixture)
import abi_headers
import select_cases as sel

R = sel.R
GUARD = 0xA5


def guarded(k, d):
    """the four outputs with a guard row behind each"""
    return (np.full((k + 1, d), 0xA5A5A5A5, dtype=np.uint32), np.full((k + 1, d), 0xA5A5A5A5, dtype=np.uint32),
            np.full((k + 1, d, 32), GUARD, dtype=np.uint8), np.full(k + 1 + 7, GUARD, dtype=np.uint8))


def guards_intact(bufs, k):
    sp, lp, cm, ok = bufs
    return bool((sp[k] == 0xA5A5A5A5).all() and (lp[k] == 0xA5A5A5A5).all() and (cm[k] == GUARD).all() and (ok[k:] == GUARD).all())


@pytest.fixture(scope="module")
def launched(hc):
    """{label: ((set_pos, list_pos, common, ok), geometry)} of every case, each run once"""
    out = {}
    for c in sel.cases():
        k, d = c["k"], c["d"]
        bufs, geom = guarded(k, d), np.zeros(8, dtype=np.uint32)
        S, L = sel.set_rows(c), sel.list_rows(c)
        rc = hc.hc_fr_find_common(S.ctypes.data, len(c["sets"]), c["m"], L.ctypes.data, c["a"], d, k, *[b.ctypes.data for b in bufs], geom.ctypes.data)
        assert rc == 0 and guards_intact(bufs, k), c["label"]
        out[c["label"]] = (tuple(b[:k] for b in bufs), tuple(int(v) for v in geom))
    return out


# ------------------------------------------------------------------------------------------------ the case list
def test_case_list_covers_what_it_claims():
    cases = sel.cases()
    assert {c["a"] for c in cases} >= set(sel.A_SIZES) | {1024} and {c["m"] for c in cases} >= set(sel.M_SIZES) | {1024}
    for a in sel.A_SIZES:
        assert {c["m"] for c in cases if c["a"] == a} >= set(sel.M_SIZES), a
    for size, key in ((sel.A_SIZES, "a"), (sel.M_SIZES, "m")):
        for v in size:
            assert {c["shared"] for c in cases if c[key] == v} == {True, False}, (key, v)
    assert {(c["k"], c["shared"]) for c in cases} >= {(k, s) for k in sel.K_SIZES for s in (True, False)}
    assert all(len(c["sets"]) == (1 if c["shared"] else c["k"]) and len(c["lists"]) == c["k"] for c in cases)
    assert all(len(s) == c["m"] for c in cases for s in c["sets"]) and all(len(l) == c["a"] for c in cases for l in c["lists"])
    found = set()
    for c in cases:
        found |= sel.classes(c)
    assert found >= sel.CLASSES, sel.CLASSES - found
    assert "repeat of an earlier chunk's element" in sel.classes(sel.by_label("chunked")) and "kept elements on both sides of a chunk boundary" in sel.classes(sel.by_label("chunked"))
    oks = [sel.expected(c)[3] for c in cases]
    assert any(0 < o.sum() < len(o) for o in oks) and any(not o.any() for o in oks) and any(o.all() for o in oks)
    full, last = sel.by_label("limit/1024-of-1024"), sel.by_label("limit/last-to-last")
    assert sel.expected(full)[3].tolist() == [1, 0] and sorted(sel.expected(full)[0][0].tolist()) == list(range(1024))
    sp, lp, cm, ok = sel.expected(last)
    assert ok.tolist() == [1] and sp.tolist() == [[1023]] and lp.tolist() == [[1023]]
    for d, want in ((1, [1, 1, 1, 1, 1, 0]), (3, [1, 1, 1, 0, 1, 0]), (4, [1, 0, 0, 0, 0, 0])):
        sp, lp, cm, ok = sel.expected(sel.by_label("reference-table/d%d" % d))
        assert ok.tolist() == want
        if d == 3:
            assert sp[0].tolist() == [3, 1, 0] and lp[0].tolist() == [0, 2, 3] and sp[1].tolist() == [1, 2, 0] and lp[1].tolist() == [1, 5, 6]
            assert sp[4].tolist() == [5, 3, 0] and lp[4].tolist() == [0, 3, 4]


def test_expectation_is_select_common_and_the_go_function():
    """expected() against sw05.select_common (positions) and sw05_fixture.find_common (values): three restatements that share no code"""
    from gopairingbasedcryptography_amd import sw05
    from sw05_fixture import find_common
    for c in sel.cases():
        if c["m"] * c["a"] * c["k"] > 200000 and not c["label"].startswith("limit"):
            continue
        sp, lp, cm, ok = sel.expected(c)
        for j in ([None] if c["shared"] else range(c["k"])):
            lists = c["lists"] if j is None else [c["lists"][j]]
            kp, cp, okk = sw05.select_common(c["sets"][0 if j is None else j], lists, c["d"])
            pick = slice(None) if j is None else slice(j, j + 1)
            assert kp.tolist() == sp[pick].tolist() and cp.tolist() == lp[pick].tolist() and okk.tolist() == ok[pick].tolist(), c["label"]
        for j in range(c["k"]):
            S = find_common(sel.item_set(c, j), c["lists"][j], c["d"])
            assert (S is not None) == bool(ok[j]), (c["label"], j)
            if S is not None:
                assert sel.rows(S).tobytes() == cm[j].tobytes(), (c["label"], j)


# ------------------------------------------------------------------------------------------------ the kernel under bounds
def test_find_common_as_launched(launched):
    bad = []
    for c in sel.cases():
        bad += sel.mismatches(c, launched[c["label"]][0])
    assert bad == []


def test_geometry_as_launched(launched):
    """[lanes per item, items per workgroup, chunks, set pitch in words, LDS instance, shared, workgroups, active lanes]"""
    g = {label: v[1] for label, v in launched.items()}
    assert g["a24-m32-k65-shared"] == (24, 2, 1, 0, 0, 1, 33, 65 * 24) and g["a24-m32-k65-own"] == (24, 2, 1, 257, 0, 0, 33, 65 * 24)
    assert g["reference-table/d3"] == (7, 9, 1, 0, 0, 1, 1, 42) and g["chunked"] == (64, 1, 3, 521, 1, 0, 3, 192)
    assert g["limit/1024-of-1024"] == (64, 1, 16, 0, 1, 1, 2, 128) and g["d-beyond-m"][:2] == (33, 1)
    one = next(v for label, v in g.items() if label.startswith("a1-m257-"))                   # 64 lists of one element: sets of their own do not all fit
    assert one[0] == 1 and one[1] == (64 if one[5] else 3) and one[4] == 1
    assert {v[4] for v in g.values()} == {0, 1} and {v[5] for v in g.values()} == {0, 1}
    assert any(v[1] > 1 and c["k"] % v[1] and c["k"] > v[1] for c in sel.cases() for v in [g[c["label"]]])      # a last workgroup that is not full
    for c in sel.cases():
        v = g[c["label"]]
        assert v[6] == -(-c["k"] // v[1]) and v[7] == c["k"] * v[0], c["label"]


def test_harness_refuses_what_the_entry_refuses(hc):
    z = np.zeros(64 * 32, dtype=np.uint8)
    p = z.ctypes.data
    good = [p, 1, 2, p, 2, 1, 1, p, p, p, p, None]
    assert hc.hc_fr_find_common(*good) == 0
    for at, v in ((0, None), (3, None), (7, None), (8, None), (9, None), (10, None), (1, 2), (2, 0), (2, 1025), (4, 0), (4, 1025), (5, 0), (5, 1025), (6, 0)):
        args = list(good)
        args[at] = v
        assert hc.hc_fr_find_common(*args) == -1, (at, v)


# ------------------------------------------------------------------------------------------------ the header, the table, the build
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


def test_select_signature_table_is_the_select_header(lib):
    from gopairingbasedcryptography_amd import _lib
    protos = abi_headers.prototypes("gpbc_bn254_select.h")
    assert sorted(protos) == sorted(_lib.SELECT_SIGNATURES) == ["gpbc_fr_find_common", "gpbc_fr_find_common_dev", "gpbc_select_version"]
    ctype = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int}
    for name, (ret, params) in protos.items():
        assert _lib.SELECT_SIGNATURES[name] == ret + ":" + "".join(params), name
        fn = getattr(lib, name)
        assert fn.restype is ctype[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [ctype[k] for k in params], name
    assert lib.gpbc_select_version() == 1 and lib.gpbc_recon_version() == 1 and lib.gpbc_share_version() == 1 and lib.gpbc_abi_version() == 8
    assert lib.gpbc_ext_version() == 2 and lib.gpbc_subset_version() == 1 and lib.gpbc_hash_version() == 1 and lib.gpbc_indexed_version() == 1
    header = open(os.path.join(ROOT, "include", "gpbc_bn254_select.h")).read()
    assert "Entry map" in header and "utils/find_common_attributes.go:7-35" in header and "fibe/sw05_fibe_common.go:284-333" in header


def test_build_lists_cover_the_new_header_and_lane_functions():
    from gopairingbasedcryptography_amd import _build
    assert "select29.hip.hpp" in _build.HEADERS
    fr = open(os.path.join(_build.CSRC, "gpbc_fr.hip")).read()
    assert 'include "select29.hip.hpp"' in fr and "k_fr_find_common" in fr
    assert not os.path.exists(os.path.join(_build.CSRC, "gpbc_select.hip"))
    lane = open(os.path.join(_build.CSRC, "select29.hip.hpp")).read()
    assert "asm" not in lane and all(name in lane for name in ("fr_select_geometry", "fr_select_stage", "fr_select_match", "fr_select_mark", "fr_select_pick"))
    harness = open(os.path.join(ROOT, "tools", "bounds_check.cpp")).read()
    assert all(name + "(" in harness for name in ("fr_select_geometry", "fr_select_stage", "fr_select_match", "fr_select_mark", "fr_select_pick"))


# ------------------------------------------------------------------------------------------------ arguments, without a device
def test_c_entries_reject_invalid_arguments(lib):
    """GPBC_ERR_INVALID_ARG with a message, nothing written, before any device is touched"""
    ins, sp, lp, cm, ok = np.zeros(64 * 32, np.uint8), np.zeros(64, np.uint32), np.zeros(64, np.uint32), np.zeros(64 * 32, np.uint8), np.zeros(64, np.uint8)
    S, L = ins.ctypes.data, ins.ctypes.data + 32 * 32
    good = [S, 1, 4, L, 4, 2, 2, sp.ctypes.data, lp.ctypes.data, cm.ctypes.data, ok.ctypes.data]
    bad = [(0, None, b"null"), (3, None, b"null"), (7, None, b"null"), (8, None, b"null"), (9, None, b"null"), (10, None, b"null"),
           (1, 3, b"n_sets"), (1, 0, b"n_sets"), (2, 0, b"1 .. 1024"), (2, 1025, b"1 .. 1024"), (4, 0, b"1 .. 1024"), (4, 1025, b"1 .. 1024"),
           (5, 0, b"1 .. 1024"), (5, 1025, b"1 .. 1024"), (6, 1 << 29, b"too many"), (6, (1 << 64) - 1, b"too many"),
           (7, S, b"overlaps"), (9, L + 32, b"overlaps"), (8, sp.ctypes.data + 4, b"overlaps"), (10, cm.ctypes.data + 100, b"overlaps"), (10, L + 255, b"overlaps")]
    for fn, extra in ((lib.gpbc_fr_find_common, []), (lib.gpbc_fr_find_common_dev, [None])):
        for at, v, why in bad:
            args = list(good)
            args[at] = v
            assert fn(*args, *extra) == -1 and why in lib.gpbc_last_error(), (at, v, lib.gpbc_last_error())
        zero = list(good)
        zero[6] = 0
        assert fn(*zero, *extra) == 0                                                             # k == 0: nothing to do, whatever the pointers
        zero[0] = zero[7] = None
        assert fn(*zero, *extra) == 0
    assert not ins.any() and not sp.any() and not lp.any() and not cm.any() and not ok.any()


def test_wrapper_rejects_malformed_arguments():
    """ValueError before any C call"""
    import torch
    from gopairingbasedcryptography_amd import bn254
    z = lambda n: np.zeros(n, dtype=np.uint8)
    S, L, buf = z(4 * 32), z(2 * 3 * 32), z(64 * 32)
    call = lambda *a, **kw: (lambda: bn254.fr_find_common(*a, **kw))
    bad = [
        (call(S, L, 0, 3, 2), "m must be in 1 .. 1024"), (call(S, L, 4, 1025, 2), "a must be in 1 .. 1024"), (call(S, L, 4, 3, True), "d must be"),
        (call(S, L, 4, 3, 2.0), "d must be"), (call([1, 2, 3, 4], L, 4, 3, 2), "sets must be a uint8 array"), (call(S, [[1, 2, 3]], 4, 3, 2), "lists must be"),
        (call(S.view(np.int8), L, 4, 3, 2), "sets must be uint8"), (call(S, L.astype(np.int32), 4, 3, 2), "lists must be uint8"),
        (call(S[:-1], L, 4, 3, 2), "whole number of rows"), (call(S, L, 3, 3, 2), "whole sets"), (call(S, L, 4, 4, 2), "whole lists"),
        (call(z(0), L, 4, 3, 2), "whole sets"), (call(z(3 * 4 * 32), L, 4, 3, 2), "one set or one per list"),
        (call(torch.zeros(4 * 32, dtype=torch.uint8), L, 4, 3, 2), "all be CUDA tensors or all host"),
        (call(S, L, 4, 3, 2, common_out=torch.zeros(2 * 2 * 32, dtype=torch.uint8)), "all be CUDA tensors or all host"),
        (call(S, L, 4, 3, 2, set_pos_out=z(2 * 2 * 4 - 1)), "set_pos_out must be"), (call(S, L, 4, 3, 2, list_pos_out=np.zeros(4, np.int32)), "list_pos_out must be"),
        (call(S, L, 4, 3, 2, common_out=z(2 * 2 * 32 + 1)), "common_out must be"), (call(S, L, 4, 3, 2, ok_out=z(3)), "ok_out must be"),
        (call(S, L, 4, 3, 2, set_pos_out=buf[1:17]), "4-byte aligned"),
        (call(buf[:128], L, 4, 3, 2, common_out=buf[64:192]), "overlaps"), (call(S, buf[:192], 4, 3, 2, ok_out=buf[190:192]), "overlaps"),
        (call(S, L, 4, 3, 2, set_pos_out=buf[:16], list_pos_out=buf[12:28]), "overlaps"), (call(S, L, 4, 3, 2, common_out=buf[:128], ok_out=buf[127:129]), "overlaps"),
    ]
    for fn, why in bad:
        with pytest.raises(ValueError, match=why):
            fn()
    sp, lp, cm, ok = bn254.fr_find_common(S, z(0), 4, 3, 2)                                        # no items: nothing to do
    assert sp.shape == lp.shape == (0, 2) and sp.dtype == np.int32 and cm.shape == (0, 2, 32) and ok.shape == (0,)


def test_no_cpu_fallback_for_find_common(lib):
    """without a GPU nothing computes the selection in the kernel's place"""
    import torch
    from gopairingbasedcryptography_amd import bn254, EngineError
    c = sel.by_label("reference-table/d3")
    if torch.cuda.is_available():
        assert sel.mismatches(c, bn254.fr_find_common(sel.set_rows(c), sel.list_rows(c), c["m"], c["a"], c["d"])) == []
        return
    with pytest.raises(EngineError):
        bn254.fr_find_common(sel.set_rows(c), sel.list_rows(c), c["m"], c["a"], c["d"])
    sp, lp, cm, ok = guarded(c["k"], c["d"])
    S, L = sel.set_rows(c), sel.list_rows(c)
    assert lib.gpbc_fr_find_common(S.ctypes.data, 1, c["m"], L.ctypes.data, c["a"], c["d"], c["k"], sp.ctypes.data, lp.ctypes.data, cm.ctypes.data, ok.ctypes.data) < 0
    assert (sp == 0xA5A5A5A5).all() and (cm == GUARD).all() and (ok == GUARD).all() and lib.gpbc_last_error()
