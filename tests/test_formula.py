"""LSSS matrices and 0 / 1 weights from boolean formulas (csrc/formula29.hip.hpp; csrc/gpbc_fr.hip: k_fr_lsss_from_formula,
k_formula_select; include/gpbc_bn254_formula.h), CPU part.

The kernels as they are launched — staging into a checked stand-in for the LDS block, the walks and the write-out behind it workgroup by
workgroup — compiled for the host with -DGPBC_BOUNDS (tools/bounds_check.cpp: hc_fr_lsss_from_formula, hc_formula_select), against the
recursive restatement of tests/formula_cases.py on every case, exactly, with a guard row behind every output.  Then the contract between
the two entries and FindLinearCombinationWeight (lw11.reconstruction_weights), formula.py against the same restatement, the new header
against _lib.FORMULA_SIGNATURES, the build's dependency lists, and the argument checks that need no device."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from bounds_harness import hc  # noqa: F401  (the fixture)
import abi_headers
import formula_cases as fc

GUARD = 0xA5
BUILD, SELECT = fc.build_cases(), fc.select_cases()


def aligned(n, shift=0):
    """n guard bytes starting `shift` bytes behind a 16-byte boundary"""
    raw = np.full(n + 32, GUARD, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16 + shift
    return raw[off:off + n]


def build_buffers(k, rows, cols, shift=0):
    """the four outputs with a guard row behind each"""
    return (aligned((k + 1) * rows * cols * 32, shift), np.full((k + 1, rows), 0x5A5A5A5A5A5A5A5A, dtype=np.int64), np.full((k + 1, 2), 0xA5A5A5A5, dtype=np.uint32),
            np.full(k + 8, GUARD, dtype=np.uint8))


def build_mismatches(c, got, bufs=None):
    """labels of what differs from the restatement; with the guarded buffers also the guard rows"""
    k, rows, cols = len(c["trees"]), c["rows"], c["cols"]
    matrix, rho, dims, ok = fc.expected_build(c)
    bad = []
    for name, g, w in (("matrix", got[0], matrix), ("rho", got[1], rho), ("dims", got[2], dims), ("ok", got[3], ok)):
        g = np.asarray(g)
        if g.shape != w.shape or not (g.astype(np.int64) == w.astype(np.int64)).all():
            bad.append("%s: %s" % (c["label"], name))
    if bufs is not None:
        m, r, d, o = bufs
        if not ((m[k * rows * cols * 32:] == GUARD).all() and (r[k] == 0x5A5A5A5A5A5A5A5A).all() and (d[k] == 0xA5A5A5A5).all() and (o[k:] == GUARD).all()):
            bad.append("%s: guard" % c["label"])
    return bad


def select_mismatches(c, got):
    chosen, ok = fc.expected_select(c)
    return ["%s: %s" % (c["label"], name) for name, g, w in (("chosen", got[0], chosen), ("ok", got[1], ok)) if np.asarray(g).shape != w.shape or not (np.asarray(g) == w).all()]


# ------------------------------------------------------------------------------------------------ the case list
def test_case_list_covers_what_it_claims():
    assert [len(fc.all_formulas(n)) for n in (1, 2, 3, 4)] == [1, 2, 8, 40] and len(fc.UP_TO_4) == 51
    assert len({tuple(fc.preorder(f)) for f in fc.UP_TO_4}) == 51
    m, rho = fc.matrix_of(("and", 1, 2))
    assert m == [[0, -1], [1, 1]] and rho == [1, 2]                                # left and right pinned
    assert fc.matrix_of(7) == ([[1]], [7]) and fc.matrix_of(("or", 1, 2)) == ([[1], [1]], [1, 2])
    assert fc.matrix_of(("or", ("and", 1, 2), 3)) == ([[0, -1], [1, 1], [1, 0]], [1, 2, 3])
    for tree, cols in zip(fc.BIG, (64, 64, 1, 1, 22)):
        m, rho = fc.matrix_of(tree)
        assert len(m) == 64 and len(m[0]) == cols and len(fc.preorder(tree)) == 127
        assert fc.choose(tree, [1] * 64)[0]
    rag = fc.ragged()
    assert len(rag) == 67 and sorted({fc.n_leaves(t) for t in rag}) == list(range(1, 65))
    ok = fc.expected_build(fc.by_label(BUILD, "ragged/16x8"))[3]
    assert 0 < ok.sum() < len(ok) and fc.expected_build(fc.by_label(BUILD, "ragged/64x64"))[3].all()
    over_rows = [t for t in rag if fc.n_leaves(t) > 16]
    over_cols = [t for t in rag if fc.n_leaves(t) <= 16 and len(fc.matrix_of(t)[0][0]) > 8]
    assert over_rows and over_cols
    bad = fc.by_label(BUILD, "malformed")
    assert [fc.well_formed(r) for r in bad["nodes"]] == [True] + [False] * len(fc.MALFORMED) + [True]
    assert fc.expected_build(bad)[3].tolist() == [1] + [0] * len(fc.MALFORMED) + [1]
    assert all(fc.well_formed(r) for c in BUILD if c["label"] != "malformed" for r in c["nodes"])
    sub = fc.by_label(SELECT, "up-to-4/every-subset")
    assert len(sub["held"]) == 2 + 2 * 4 + 8 * 8 + 40 * 16
    oks = [fc.expected_select(c)[1] for c in SELECT]
    assert all(0 < o.sum() < len(o) for o, c in zip(oks, SELECT) if len(o) > 1)
    assert len(fc.by_label(SELECT, "shared/k130")["held"]) == 130
    rep = fc.expected_select(fc.by_label(SELECT, "repeated"))
    assert rep[0].tolist() == [[1, 1, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 1, 1], [0, 0, 0]] and rep[1].tolist() == [1, 1, 1, 0, 1, 0]


# ------------------------------------------------------------------------------------------------ the kernels under bounds
@pytest.fixture(scope="module")
def built(hc):
    """{(label, wide): (matrix, rho, dims, ok)}: every build case through the 128-bit stores and through the byte stores"""
    out, bad = {}, []
    for c in BUILD:
        k, rows, cols = len(c["trees"]), c["rows"], c["cols"]
        for wide, shift in ((1, 0), (0, 3)):
            bufs, geom = build_buffers(k, rows, cols, shift), np.zeros(4, dtype=np.uint32)
            nodes = np.ascontiguousarray(c["nodes"])
            rc = hc.hc_fr_lsss_from_formula(nodes.ctypes.data, c["N"], k, rows, cols, *[b.ctypes.data for b in bufs], wide, geom.ctypes.data)
            assert rc == 0, (c["label"], wide)
            assert geom.tolist() == [1, 769, k, k * rows * cols * 2]
            got = (bufs[0][:k * rows * cols * 32].reshape(k, rows, cols, 32), bufs[1][:k], bufs[2][:k], bufs[3][:k])
            bad += build_mismatches(c, got, bufs)
            out[c["label"], wide] = got
    assert bad == []
    return out


def test_from_formula_as_launched(built):
    assert len(built) == 2 * len(BUILD)
    for c in BUILD:
        assert built[c["label"], 1][0].tobytes() == built[c["label"], 0][0].tobytes()


@pytest.fixture(scope="module")
def selected(hc):
    out, bad = {}, []
    for c in SELECT:
        k, rows = len(c["held"]), c["rows"]
        chosen, ok, geom = np.full((k + 1, rows), GUARD, dtype=np.uint8), np.full(k + 8, GUARD, dtype=np.uint8), np.zeros(4, dtype=np.uint32)
        nodes, held = np.ascontiguousarray(c["nodes"]), np.ascontiguousarray(c["held"])
        rc = hc.hc_formula_select(nodes.ctypes.data, len(nodes), c["N"], held.ctypes.data, k, rows, chosen.ctypes.data, ok.ctypes.data, geom.ctypes.data)
        assert rc == 0 and (chosen[k] == GUARD).all() and (ok[k:] == GUARD).all(), c["label"]
        shared = c["shared"] and k > 1
        assert geom.tolist() == ([64, 0, 1, -(-k // 64)] if shared else [16, 255, 0, -(-k // 16)]), c["label"]
        bad += select_mismatches(c, (chosen[:k], ok[:k]))
        out[c["label"]] = (chosen[:k], ok[:k])
    assert bad == []
    return out


def test_formula_select_as_launched(selected):
    assert len(selected) == len(SELECT)


def test_chosen_rows_sum_to_e0_and_ok_is_the_field_solve(selected):
    """for every item: chosen <= held; with ok = 1 the chosen rows of the formula's matrix sum to (1, 0, ..., 0) modulo r; and ok is
    whether FindLinearCombinationWeight finds weights over the held rows at all"""
    from gopairingbasedcryptography_amd import lw11
    solved = {}
    for c in SELECT:
        chosen, ok = selected[c["label"]]
        for j in range(len(c["held"])):
            tree = c["trees"][0 if c["shared"] else j]
            if tree is None or fc.n_leaves(tree) > c["rows"]:
                assert not ok[j] and not chosen[j].any()
                continue
            m, _ = fc.matrix_of(tree)
            held = [x for x in range(len(m)) if c["held"][j][x]]
            assert not (chosen[j] & (c["held"][j] == 0)).any() and not chosen[j, len(m):].any()
            key = (id(tree), tuple(held))
            if key not in solved:
                solved[key] = lw11.reconstruction_weights(m, list(range(len(m))), held) is not None
            assert bool(ok[j]) == solved[key], (c["label"], j)
            if ok[j]:
                total = [sum(m[x][y] for x in range(len(m)) if chosen[j][x]) % fc.R for y in range(len(m[0]))]
                assert total == [1] + [0] * (len(m[0]) - 1), (c["label"], j)


def test_harness_refuses_what_the_entries_refuse(hc):
    n, out = np.array([[fc.OR, 1, 2]], dtype=np.int64), aligned(4096)
    r, d, o, h = np.zeros(8, np.int64), np.zeros(2, np.uint32), np.zeros(8, np.uint8), np.ones(8, np.uint8)
    good = [n.ctypes.data, 3, 1, 2, 1, out.ctypes.data, r.ctypes.data, d.ctypes.data, o.ctypes.data, 1, None]
    assert hc.hc_fr_lsss_from_formula(*good) == 0
    nodims = list(good)
    nodims[7] = None
    assert hc.hc_fr_lsss_from_formula(*nodims) == 0
    for at, v in ((0, None), (5, None), (6, None), (8, None), (1, 0), (1, 128), (2, 0), (3, 0), (3, 65), (4, 0), (4, 65), (5, out.ctypes.data + 4)):
        args = list(good)
        args[at] = v
        assert hc.hc_fr_lsss_from_formula(*args) == -1, (at, v)
    good = [n.ctypes.data, 1, 3, h.ctypes.data, 1, 2, out.ctypes.data, o.ctypes.data, None]
    assert hc.hc_formula_select(*good) == 0
    for at, v in ((0, None), (3, None), (6, None), (7, None), (1, 2), (1, 0), (2, 0), (2, 128), (4, 0), (5, 0), (5, 65)):
        args = list(good)
        args[at] = v
        assert hc.hc_formula_select(*args) == -1, (at, v)


# ------------------------------------------------------------------------------------------------ formula.py
def test_encode_is_the_preorder_walk():
    from gopairingbasedcryptography_amd import formula
    assert (formula.AND, formula.OR, formula.END) == (fc.AND, fc.OR, fc.END) == (-2, -3, -1)
    for c in BUILD:
        if c["label"] != "malformed":
            assert formula.encode(c["trees"], c["N"]).tolist() == c["nodes"].tolist(), c["label"]
    t = ("and", 1, ("or", 2, 3))
    assert formula.encode([t, 4, t]).tolist() == [[-2, 1, -3, 2, 3], [4, -1, -1, -1, -1], [-2, 1, -3, 2, 3]]
    assert formula.encode([("AND", 1, 2)]).tolist() == [[-2, 1, 2]] and formula.encode([]).shape == (0, 1)
    # an iterable that yields fresh objects: a freed tuple's id comes back, and must not bring an earlier formula's codes with it
    fresh = lambda: (("and", 1000 + j, ("or", 2000 + j, 3000 + j)) for j in range(40))
    assert formula.encode(fresh()).tolist() == formula.encode(list(fresh())).tolist() == [[-2, 1000 + j, -3, 2000 + j, 3000 + j] for j in range(40)]
    assert formula.encode(iter([t, 4, t])).tolist() == formula.encode([t, 4, t]).tolist()
    for bad in ([("and", 1)], [("xor", 1, 2)], [-1], [1 << 63], [True], ["a"], [fc.deep("or", 65, True)]):
        with pytest.raises(ValueError):
            formula.encode(bad)
    with pytest.raises(ValueError):
        formula.encode([t], 4)
    with pytest.raises(ValueError):
        formula.encode([t], 128)


def test_check_leaves_size_and_lsss_matrix_are_the_restatement():
    from gopairingbasedcryptography_amd import formula
    for c in BUILD:
        nodes = c["nodes"]
        assert formula.check(nodes).tolist() == [int(fc.well_formed(r)) for r in nodes], c["label"]
        if c["label"] == "malformed":
            with pytest.raises(ValueError, match="malformed"):
                formula.leaves(nodes)
            with pytest.raises(ValueError, match="malformed"):
                formula.size(nodes)
            want = fc.expected_build(c)[1]
            assert formula.leaves(nodes, c["rows"], strict=False).tolist() == want.tolist()
            continue
        mats = [fc.matrix_of(t) for t in c["trees"]]
        R, C = max(len(m) for m, _ in mats), max(len(m[0]) for m, _ in mats)
        assert formula.size(nodes) == (R, C), c["label"]
        table = formula.leaves(nodes)
        assert table.shape == (len(nodes), R) and table.dtype == np.int64
        assert table.tolist() == [rho + [-1] * (R - len(rho)) for _, rho in mats], c["label"]
        if R <= c["rows"]:
            assert formula.leaves(nodes, c["rows"]).tolist() == fc.expected_build(dict(c, cols=64))[1].tolist()
        else:
            with pytest.raises(ValueError, match="more than"):
                formula.leaves(nodes, c["rows"])
            loose = formula.leaves(nodes, c["rows"], strict=False)
            assert loose.tolist() == fc.expected_build(dict(c, cols=64))[1].tolist()
        for t, row, (m, rho) in zip(c["trees"], nodes, mats):
            want = ([[v % fc.R for v in r] for r in m], rho)
            assert formula.lsss_matrix(t) == want and formula.lsss_matrix(row) == want
    assert formula.check(np.array([5], dtype=np.int64)).tolist() == [1]
    with pytest.raises(ValueError):
        formula.check(np.zeros((1, 128), dtype=np.int64))
    with pytest.raises(ValueError):
        formula.check(np.zeros((1, 3), dtype=np.int32))
    with pytest.raises(ValueError):
        formula.lsss_matrix(np.array([[fc.AND, 1, fc.END]], dtype=np.int64))


def test_lsss_matrix_feeds_reconstruction_weights():
    from gopairingbasedcryptography_amd import formula, lw11
    m, rho = formula.lsss_matrix(("or", ("and", 1, 2), ("and", 3, 4)))
    assert lw11.reconstruction_weights(m, rho, {1, 2}) == ([0, 1], [1, 1]) and lw11.reconstruction_weights(m, rho, {3, 4}) == ([2, 3], [1, 1])
    assert lw11.reconstruction_weights(m, rho, {1, 3}) is None


# ------------------------------------------------------------------------------------------------ the header, the table, the build
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


def test_formula_signature_table_is_the_formula_header(lib):
    from gopairingbasedcryptography_amd import _lib
    protos = abi_headers.prototypes("gpbc_bn254_formula.h")
    names = ["gpbc_formula_select", "gpbc_formula_select_dev", "gpbc_formula_version", "gpbc_fr_lsss_from_formula", "gpbc_fr_lsss_from_formula_dev"]
    assert sorted(protos) == sorted(_lib.FORMULA_SIGNATURES) == names
    ctype = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int}
    for name, (ret, params) in protos.items():
        assert _lib.FORMULA_SIGNATURES[name] == ret + ":" + "".join(params), name
        fn = getattr(lib, name)
        assert fn.restype is ctype[ret] and list(fn.argtypes) == [ctype[k] for k in params], name
    assert lib.gpbc_formula_version() == 1 and lib.gpbc_select_version() == 1 and lib.gpbc_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "gpbc_bn254_formula.h")).read()
    assert "Entry map" in header and "lewko_waters_lsss_matrix.go:34-87" in header
    for name, value in (("END", -1), ("AND", -2), ("OR", -3)):
        assert "#define GPBC_FORMULA_%s (%d)" % (name, value) in header


def test_build_lists_cover_the_new_header_and_lane_functions():
    from gopairingbasedcryptography_amd import _build
    assert "formula29.hip.hpp" in _build.HEADERS and not os.path.exists(os.path.join(_build.CSRC, "gpbc_formula.hip"))
    fr = open(os.path.join(_build.CSRC, "gpbc_fr.hip")).read()
    assert 'include "formula29.hip.hpp"' in fr and "k_fr_lsss_from_formula" in fr and "k_formula_select" in fr
    lane = open(os.path.join(_build.CSRC, "formula29.hip.hpp")).read()
    names = ("formula_stage", "formula_build_walk", "formula_build_write", "formula_select_lane")
    assert "asm" not in lane and all(name in lane for name in names)
    for tool in ("bounds_check.cpp", "formula_san.cpp"):
        text = open(os.path.join(ROOT, "tools", tool)).read()
        assert all(name + "(" in text for name in names), tool


# ------------------------------------------------------------------------------------------------ arguments, without a device
def test_c_entries_reject_invalid_arguments(lib):
    """GPBC_ERR_INVALID_ARG with a message, nothing written, before any device is touched"""
    nodes, mat, rho, dims, ok = np.full(64, -1, np.int64), np.zeros(4096, np.uint8), np.zeros(64, np.int64), np.zeros(64, np.uint32), np.zeros(64, np.uint8)
    N, M, Rh, D, O = nodes.ctypes.data, mat.ctypes.data, rho.ctypes.data, dims.ctypes.data, ok.ctypes.data
    good = [N, 3, 2, 2, 2, M, Rh, D, O]                                                        # k = 2 formulas of 3 nodes, 2 x 2
    bad = [(0, None, b"null"), (5, None, b"null"), (6, None, b"null"), (8, None, b"null"), (1, 0, b"n_nodes"), (1, 128, b"n_nodes"),
           (3, 0, b"1 .. 64"), (3, 65, b"1 .. 64"), (4, 0, b"1 .. 64"), (4, 65, b"1 .. 64"), (2, 1 << 29, b"too many"), (2, (1 << 64) - 1, b"too many"),
           (5, N + 40, b"overlaps"), (6, M + 248, b"overlaps"), (7, Rh + 24, b"overlaps"), (8, D + 15, b"overlaps"), (8, M, b"overlaps"), (6, N, b"overlaps")]
    for fn, extra in ((lib.gpbc_fr_lsss_from_formula, []), (lib.gpbc_fr_lsss_from_formula_dev, [None])):
        for at, v, why in bad:
            args = list(good)
            args[at] = v
            assert fn(*args, *extra) == -1 and why in lib.gpbc_last_error(), (at, v, lib.gpbc_last_error())
        zero = list(good)
        zero[2] = 0
        assert fn(*zero, *extra) == 0                                                             # k == 0: nothing to do, whatever the pointers
        zero[0] = zero[5] = None
        assert fn(*zero, *extra) == 0
    held, chosen = np.ones(64, np.uint8), np.zeros(64, np.uint8)
    H, C = held.ctypes.data, chosen.ctypes.data
    good = [N, 1, 3, H, 4, 2, C, O]                                                            # one formula, k = 4 masks of 2 rows
    bad = [(0, None, b"null"), (3, None, b"null"), (6, None, b"null"), (7, None, b"null"), (1, 0, b"n_formulas"), (1, 3, b"n_formulas"),
           (2, 0, b"n_nodes"), (2, 128, b"n_nodes"), (5, 0, b"1 .. 64"), (5, 65, b"1 .. 64"), (4, 1 << 29, b"too many"),
           (6, H + 7, b"overlaps"), (6, N + 16, b"overlaps"), (7, H, b"overlaps"), (7, C + 7, b"overlaps"), (7, N + 23, b"overlaps")]
    for fn, extra in ((lib.gpbc_formula_select, []), (lib.gpbc_formula_select_dev, [None])):
        for at, v, why in bad:
            args = list(good)
            args[at] = v
            assert fn(*args, *extra) == -1 and why in lib.gpbc_last_error(), (at, v, lib.gpbc_last_error())
        zero = list(good)
        zero[4] = 0
        assert fn(*zero, *extra) == 0
        zero[0] = zero[6] = None
        assert fn(*zero, *extra) == 0
    assert (nodes == -1).all() and not mat.any() and not rho.any() and not dims.any() and not ok.any() and not chosen.any() and held.all()


def test_wrappers_reject_malformed_arguments():
    """ValueError before any C call"""
    import torch
    from gopairingbasedcryptography_amd import bn254
    nodes, held = np.array([[fc.OR, 1, 2], [fc.AND, 1, 2]], dtype=np.int64), np.ones((2, 2), dtype=np.uint8)
    z = lambda n: np.zeros(n, dtype=np.uint8)
    build = lambda *a, **kw: (lambda: bn254.fr_lsss_from_formula(*a, **kw))
    select = lambda *a, **kw: (lambda: bn254.formula_select(*a, **kw))
    buf = z(4096)
    bad = [
        (build(nodes, 0, 2), "rows must be in 1 .. 64"), (build(nodes, 2, 65), "cols must be in 1 .. 64"), (build(nodes, True, 2), "rows must be"),
        (build(nodes.astype(np.int32), 2, 2), "nodes must be int64"), (build([[1]], 2, 2), "nodes must be an int64 array"),
        (build(np.zeros((1, 128), np.int64), 2, 2), "N in 1 .. 127"), (build(np.zeros((1, 1, 3), np.int64), 2, 2), "nodes must be"),
        (build(torch.zeros((2, 3), dtype=torch.int32), 2, 2), "contiguous int64 tensor"),
        (build(nodes, 2, 2, matrix_out=z(2 * 2 * 2 * 32 + 1)), "matrix_out must be"), (build(nodes, 2, 2, rho_out=z(31)), "rho_out must be"),
        (build(nodes, 2, 2, dims_out=z(15)), "dims_out must be"), (build(nodes, 2, 2, ok_out=z(3)), "ok_out must be"),
        (build(nodes, 2, 2, ok_out=torch.zeros(2, dtype=torch.uint8)), "all be CUDA tensors or all host"),
        (build(nodes, 2, 2, rho_out=buf[1:33]), "aligned"),
        (build(nodes, 2, 2, matrix_out=buf[:256], rho_out=buf[248:280]), "overlaps"), (build(nodes, 2, 2, dims_out=buf[:16], ok_out=buf[15:17]), "overlaps"),
        (build(nodes, 2, 2, matrix_out=buf[:256], ok_out=buf[255:257]), "overlaps"),
        (select(nodes, held, 0), "rows must be in 1 .. 64"), (select(nodes.astype(np.uint64), held, 2), "nodes must be int64"),
        (select(nodes, held.astype(np.int32), 2), "held must be uint8 or bool"), (select(nodes, [[1, 1]], 2), "held must be"),
        (select(nodes, z(5), 2), "held needs 2 bytes"), (select(nodes, z(6), 2), "one formula or one per mask"),
        (select(nodes, torch.ones(4, dtype=torch.uint8), 2), "all be CUDA tensors or all host"),
        (select(nodes, held, 2, chosen_out=z(5)), "chosen_out must be"), (select(nodes, held, 2, ok_out=z(1)), "ok_out must be"),
        (select(nodes, buf[:4], 2, chosen_out=buf[2:6]), "overlaps"), (select(nodes, held, 2, chosen_out=buf[:4], ok_out=buf[3:5]), "overlaps"),
    ]
    for fn, why in bad:
        with pytest.raises(ValueError, match=why):
            fn()
    m, rho, dims, ok = bn254.fr_lsss_from_formula(np.zeros((0, 3), dtype=np.int64), 2, 2)      # no items: nothing to do
    assert m.shape == (0, 2, 2, 32) and rho.shape == (0, 2) and rho.dtype == np.int64 and dims.shape == (0, 2) and ok.shape == (0,)
    chosen, ok = bn254.formula_select(nodes[0], z(0), 2)
    assert chosen.shape == (0, 2) and ok.shape == (0,)


def test_no_cpu_fallback_for_formulas(lib):
    """without a GPU nothing computes the matrix or the selection in the kernels' place"""
    import torch
    from gopairingbasedcryptography_amd import bn254, EngineError
    c, s = fc.by_label(BUILD, "up-to-4"), fc.by_label(SELECT, "repeated")
    if torch.cuda.is_available():
        assert build_mismatches(c, bn254.fr_lsss_from_formula(c["nodes"], c["rows"], c["cols"])) == []
        assert select_mismatches(s, bn254.formula_select(s["nodes"], s["held"], s["rows"])) == []
        return
    with pytest.raises(EngineError):
        bn254.fr_lsss_from_formula(c["nodes"], c["rows"], c["cols"])
    with pytest.raises(EngineError):
        bn254.formula_select(s["nodes"], s["held"], s["rows"])
    k = len(c["trees"])
    bufs = build_buffers(k, c["rows"], c["cols"])
    assert lib.gpbc_fr_lsss_from_formula(c["nodes"].ctypes.data, c["N"], k, c["rows"], c["cols"], *[b.ctypes.data for b in bufs]) < 0
    assert (bufs[0] == GUARD).all() and (bufs[1] == 0x5A5A5A5A5A5A5A5A).all() and (bufs[3] == GUARD).all() and lib.gpbc_last_error()
