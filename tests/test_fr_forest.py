"""Threshold-tree forests in Fr (csrc/forest29.hip.hpp; csrc/gpbc_fr.hip: k_fr_share_forest, k_fr_forest_weights;
include/gpbc_bn254_forest.h), CPU part.

Both kernels as they are launched — the plan of every tree, the check of the concatenated block, the geometry from the forest's maxima, the
item mapping, staging into a checked stand-in for the LDS block, every level to the forest's depth workgroup by workgroup, the finish —
compiled for the host with -DGPBC_BOUNDS (tools/bounds_check.cpp: hc_fr_share_forest, hc_fr_forest_weights) against Python integers on
every case of tests/forest_cases.py, exactly, with guard rows behind the outputs.  Every product in that build asserts its int64 columns
for ANY input of its interval class and every canonical form its input range, so a run that finishes is the overflow proof.  Then the new
header against _lib.FOREST_SIGNATURES, the build's dependency lists, create's refusals with their messages, and the argument checks that
need no device."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from bounds_harness import hc  # noqa: F401  (the fixture)
import abi_headers
import fr_cases as fc
import share_cases as sc
import forest_cases as fo

VP, SZ = ctypes.c_void_p, ctypes.c_size_t
R = fc.R
GUARD = 0xA5


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


@pytest.fixture(scope="module")
def launched(hc):
    """{label: (shares, valid, share geometry, w, ok, weights geometry)} of every case, each entry run once with a guard row behind both
    of its outputs"""
    out = {}
    for c in fo.cases():
        k, L = c["k"], c["Lmax"]
        res = []
        for entry in ("share", "weights"):
            rows, ok, geom = np.full((k * L + 1, 32), GUARD, dtype=np.uint8), np.full(k + 1, GUARD, dtype=np.uint8), np.zeros(8, dtype=np.uint32)
            head = (c["nodes"].ctypes.data, c["node_off"].ctypes.data, c["T"], c["tree_of"].ctypes.data)
            if entry == "share":
                rc = hc.hc_fr_share_forest(*head, c["secrets"].ctypes.data, _ptr(c["coeffs"]), k, rows.ctypes.data, ok.ctypes.data, geom.ctypes.data)
            else:
                rc = hc.hc_fr_forest_weights(*head, c["held"].ctypes.data, k, rows.ctypes.data, ok.ctypes.data, geom.ctypes.data)
            assert rc == 0, (c["label"], entry)
            assert (rows[k * L] == GUARD).all() and ok[k] == GUARD and (geom[0], geom[1]) == (L, c["Cmax"]), (c["label"], entry)
            res += [rows[:k * L], ok[:k], tuple(int(v) for v in geom)]
        out[c["label"]] = tuple(res)
    return out


# ------------------------------------------------------------------------------------------------ the case list
def test_case_list_covers_what_it_claims(launched):
    cases = fo.cases()
    assert {c["k"] for c in cases} >= {1, 3, 65, 130}
    assert {l for c in cases for l in c["labels"]} == {"leaf", "2-of-3", "example", "chain8", "16x16", "65-of-65", "many-gates", "largest"}
    assert next(c for c in cases if c["label"] == "largest/1")["k"] == 1
    assert {int(v) for c in cases for v in np.unique(c["held"])} == {0, 0x01, 0x80, 0xFF}
    seen = set()
    for c in cases:
        T, ids = c["T"], [int(t) for t in c["tree_of"]]
        if 0 < sum(c["want_ok"]) < sum(c["want_valid"]):
            seen.add("satisfied and unsatisfied items in one call")
        if T in ids and 0xFFFFFFFF in ids:
            seen.add("the ids T and 0xffffffff")
            assert 0 < sum(c["want_valid"]) < c["k"]
        used = {c["labels"][t] for t in ids if t < T}
        if "leaf" in used and len(used) > 1:
            seen.add("a one-leaf tree beside gated trees")
        # neighbours belong to different trees, so every workgroup of more than one item mixes trees and depths
        assert all(a != b for a, b in zip(ids, ids[1:])), c["label"]
        for i, t in enumerate(ids):
            Lt, Ct = (c["L"][t], c["C"][t]) if t < T else (0, 0)
            assert c["held"][i, Lt:].all() and (c["coeffs"][i, Ct:] != 0).all(), (c["label"], i)        # garbage where nothing may be read
            assert not any(c["want_shares"][i * c["Lmax"] + Lt:(i + 1) * c["Lmax"]]) and not any(c["want_w"][i * c["Lmax"] + Lt:(i + 1) * c["Lmax"]])
    for label, v in launched.items():
        for geom in (v[2], v[5]):
            seen.add("the large LDS instance" if geom[6] else "the small LDS instance")
            if geom[3] > 1:
                seen.add("several items in a workgroup")
    assert seen == {"satisfied and unsatisfied items in one call", "the ids T and 0xffffffff", "a one-leaf tree beside gated trees", "the small LDS instance",
                    "the large LDS instance", "several items in a workgroup"}


def test_expectations_recombine():
    """the two halves of the expectation agree: sum_y w_y share_y is the item's secret wherever ok = 1, on the padded rows"""
    n = 0
    for c in fo.cases():
        secrets, L = fc.ints(c["secrets"]), c["Lmax"]
        for i in range(c["k"]):
            if c["want_ok"][i]:
                assert sum(a * b for a, b in zip(c["want_w"][i * L:(i + 1) * L], c["want_shares"][i * L:(i + 1) * L])) % R == secrets[i] % R, (c["label"], i)
                n += 1
    assert n > 100


# ------------------------------------------------------------------------------------------------ the kernels under bounds
def test_share_forest_as_launched(launched):
    assert fo.run_share(lambda c: launched[c["label"]][:2], fo.cases()) == []


def test_forest_weights_as_launched(launched):
    assert fo.run_weights(lambda c: launched[c["label"]][3:5], fo.cases()) == []


def test_padded_columns_are_zero_and_unknown_trees_give_zero_rows(launched):
    for c in fo.cases():
        k, L = c["k"], c["Lmax"]
        for rows in (launched[c["label"]][0], launched[c["label"]][3]):
            rows = rows.reshape(k, L, 32)
            for i, t in enumerate(int(t) for t in c["tree_of"]):
                Lt = c["L"][t] if t < c["T"] else 0
                assert not rows[i, Lt:].any(), (c["label"], i)
        bad = [i for i, t in enumerate(c["tree_of"]) if t >= c["T"]]
        assert not launched[c["label"]][1][bad].any() and not launched[c["label"]][4][bad].any()


def test_geometry_as_launched(launched):
    """[Lmax, Cmax, depth, items per workgroup, lanes per item, words per item, LDS instance, workgroups] from the forest's maxima alone"""
    g = {label: (v[2], v[5]) for label, v in launched.items()}
    assert g["mixed/130"] == ((65, 64, 8, 4, 16, 65 * 9, 0, 33), (65, 64, 8, 16, 4, 93, 0, 9))
    assert g["mixed/1"][0][3:7] == g["mixed/130"][0][3:7] and g["mixed/bad-ids"][1][3:7] == g["mixed/130"][1][3:7]      # not a function of k or tree_of
    assert g["edge/65"] == ((256, 255, 8, 1, 64, 272 * 9 + 1, 0, 65), (256, 255, 8, 4, 16, 443, 0, 17))
    assert g["large/11"] == ((512, 273, 3, 2, 32, 546 * 9 + 1, 1, 6), (512, 273, 3, 2, 32, 3515, 1, 6))
    assert g["largest/1"] == ((1024, 2, 2, 1, 64, 1026 * 9 + 1, 1, 1), (1024, 2, 2, 1, 64, 12289, 1, 1))
    for share, recon in g.values():
        assert share[3] * share[4] == 64 and recon[3] * recon[4] == 64


def test_a_forest_of_one_tree_is_that_tree(hc):
    """the forest entries on T = 1 against the single-tree entries of the same harness, byte for byte (alternating; many-gates: the large
    instance of both)"""
    import tree_weight_cases as tw
    for label, k in (("alternating", 9), ("many-gates", 3)):
        c = next(c for c in tw.cases() if c["label"] == label)
        nodes, L, C = c["nodes"], c["L"], sc.n_coeffs(c["tree"])
        off, ids = np.array([0, len(nodes)], dtype=np.uint32), np.zeros(k, dtype=np.uint32)
        secrets, coeffs, held = fc.rows(sc.rand("one-s-" + label, k)), fc.rows(sc.rand("one-q-" + label, k * C)), np.ascontiguousarray(c["held"][:k])
        a, b, oka, okb = (np.zeros((k * L, 32), dtype=np.uint8) for _ in range(4))
        assert hc.hc_fr_share_tree(nodes.ctypes.data, len(nodes), secrets.ctypes.data, coeffs.ctypes.data, k, a.ctypes.data, None) == 0
        assert hc.hc_fr_share_forest(nodes.ctypes.data, off.ctypes.data, 1, ids.ctypes.data, secrets.ctypes.data, coeffs.ctypes.data, k, b.ctypes.data, None, None) == 0     # no ok wanted
        assert a.any() and (a == b).all(), label
        assert hc.hc_fr_tree_weights(nodes.ctypes.data, len(nodes), held.ctypes.data, k, a.ctypes.data, oka.ctypes.data, None) == 0
        assert hc.hc_fr_forest_weights(nodes.ctypes.data, off.ctypes.data, 1, ids.ctypes.data, held.ctypes.data, k, b.ctypes.data, okb.ctypes.data, None) == 0
        assert oka[:k, 0].any() and (a == b).all() and (oka == okb).all(), label


# ------------------------------------------------------------------------------------------------ refusals of the plan
def forest_of(lists):
    nodes = sc.node_array([n for lst in lists for n in lst])
    return nodes, np.cumsum([0] + [len(lst) for lst in lists]).astype(np.uint32)


GOOD = [(sc.ROOT_MARK, 2), (0, 0), (0, 0)]


def test_plan_refuses_with_the_tree_and_the_reason(hc):
    from gopairingbasedcryptography_amd import bn254
    why, bad = ctypes.create_string_buffer(96), SZ(0)
    for name, lst in sc.MALFORMED.items():
        if not lst:
            continue                                                                          # a tree of no nodes is a node_off that does not increase: below
        nodes, off = forest_of([GOOD, GOOD, lst, GOOD])
        assert hc.hc_fr_forest_plan(nodes.ctypes.data, off.ctypes.data, 4, None, ctypes.byref(bad), why) == -1, name
        assert bad.value == 2 and why.value.decode() == bn254.share_tree_check([tuple(int(v) for v in n) for n in lst]), name
    nodes, off = forest_of([GOOD, GOOD])
    for n_trees, offsets, tree, reason in ((0, off, 0, "at least one tree"), (65537, off, 65537, "more than 65536 trees"),
                                           (2, np.array([0, 3, 3], dtype=np.uint32), 1, "node_off must increase"), (2, np.array([3, 0, 6], dtype=np.uint32), 0, "node_off must increase")):
        assert hc.hc_fr_forest_plan(nodes.ctypes.data, offsets.ctypes.data, n_trees, None, ctypes.byref(bad), why) == -1
        assert bad.value == tree and reason in why.value.decode()
    sizes = np.zeros(10, dtype=np.uint32)
    c = next(c for c in fo.cases() if c["label"] == "mixed/130")
    assert hc.hc_fr_forest_plan(c["nodes"].ctypes.data, c["node_off"].ctypes.data, c["T"], sizes.ctypes.data, None, None) == 0
    assert sizes.tolist() == [5, 65, 8, 64, 65, 8, 1, 65, 65, 93]         # T, Lmax, Gmax, Cmax, Umax, depth, narrowest, widest level, Emax, Pmax
    z = np.zeros(64 * 32, dtype=np.uint8)
    p, ids = z.ctypes.data, np.zeros(1, dtype=np.uint32).ctypes.data
    for args in ((None, p, 1, p), (ids, None, 1, p), (ids, p, 0, p), (ids, p, 1, None)):
        assert hc.hc_fr_share_forest(nodes.ctypes.data, off.ctypes.data, 2, args[0], args[1], p, args[2], args[3], p, None) == -1, args
        assert hc.hc_fr_forest_weights(nodes.ctypes.data, off.ctypes.data, 2, args[0], args[1], args[2], args[3], p, None) == -1, args


# ------------------------------------------------------------------------------------------------ the header, the table, the build
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


def test_forest_signature_table_is_the_forest_header(lib):
    from gopairingbasedcryptography_amd import _lib
    protos = abi_headers.prototypes("gpbc_bn254_forest.h")
    assert sorted(protos) == sorted(_lib.FOREST_SIGNATURES) == sorted(
        ["gpbc_forest_version", "gpbc_share_forest_create", "gpbc_share_forest_destroy", "gpbc_share_forest_trees", "gpbc_share_forest_leaves", "gpbc_share_forest_coeffs",
         "gpbc_share_forest_tree_leaves", "gpbc_share_forest_tree_coeffs", "gpbc_fr_share_forest", "gpbc_fr_share_forest_dev", "gpbc_fr_forest_weights", "gpbc_fr_forest_weights_dev"])
    ctype = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int}
    for name, (ret, params) in protos.items():
        assert _lib.FOREST_SIGNATURES[name] == ret + ":" + "".join(params), name
        fn = getattr(lib, name)
        assert fn.restype is ctype[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [ctype[k] for k in params], name
    assert lib.gpbc_forest_version() == 1 and lib.gpbc_recon_version() == 1 and lib.gpbc_share_version() == 1 and lib.gpbc_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "gpbc_bn254_forest.h")).read()
    assert '#include "gpbc_bn254_share.h"' in header and "Entry map" in header and "tree id is out of range" in header


def test_build_lists_cover_the_new_header_and_lane_functions():
    from gopairingbasedcryptography_amd import _build
    assert "forest29.hip.hpp" in _build.HEADERS
    fr = open(os.path.join(_build.CSRC, "gpbc_fr.hip")).read()
    assert 'include "forest29.hip.hpp"' in fr and "k_fr_share_forest" in fr and "k_fr_forest_weights" in fr
    assert not os.path.exists(os.path.join(_build.CSRC, "gpbc_forest.hip"))


# ------------------------------------------------------------------------------------------------ arguments, without a device
def test_create_refuses_before_the_device_is_touched(lib):
    """GPBC_ERR_INVALID_ARG with *out = NULL and a message that names the tree and gives gpbc_share_tree_create's reason"""
    from gopairingbasedcryptography_amd import bn254
    h = VP(1)

    def create(nodes, off, n):
        h.value = 1
        rc = lib.gpbc_share_forest_create(VP(nodes.ctypes.data), VP(off.ctypes.data), SZ(n), ctypes.byref(h))
        assert h.value is None
        return rc, lib.gpbc_last_error().decode()
    for name, lst in sc.MALFORMED.items():
        if not lst:
            continue
        nodes, off = forest_of([GOOD, lst, GOOD])
        rc, msg = create(nodes, off, 3)
        assert rc == -1 and "malformed tree 1: " + bn254.share_tree_check([tuple(int(v) for v in n) for n in lst]) in msg, (name, msg)
    nodes, off = forest_of([GOOD, GOOD])
    assert create(nodes, off, 0) == (-1, "malformed forest: a forest needs at least one tree")
    assert create(nodes, off, 65537) == (-1, "malformed forest: more than 65536 trees")
    rc, msg = create(nodes, np.array([0, 3, 3], dtype=np.uint32), 2)
    assert rc == -1 and "malformed tree 1: node_off must increase" in msg
    assert lib.gpbc_share_forest_create(VP(nodes.ctypes.data), VP(off.ctypes.data), SZ(2), None) == -1 and b"null" in lib.gpbc_last_error()
    assert lib.gpbc_share_forest_create(None, VP(off.ctypes.data), SZ(2), ctypes.byref(h)) == -1 and b"null" in lib.gpbc_last_error()


def test_c_entries_reject_a_null_handle(lib):
    """GPBC_ERR_INVALID_ARG with a message, nothing written, before any device is touched.  A handle needs a device, so what can be asked
    here is the null handle, whatever else is passed (tests/test_fr_forest_gpu.py has the refusals of a live handle)."""
    buf, out, ok = np.zeros(64 * 32, np.uint8), np.zeros(64 * 32, np.uint8), np.zeros(64, np.uint8)
    p, o, q = VP(buf.ctypes.data), VP(out.ctypes.data), VP(ok.ctypes.data)
    for k in (1, 0, 1 << 29, (1 << 64) - 1):
        assert lib.gpbc_fr_share_forest(None, p, p, p, SZ(k), o, q) == -1 and b"null forest" in lib.gpbc_last_error(), k
        assert lib.gpbc_fr_share_forest_dev(None, p, p, p, SZ(k), o, q, None) == -1 and b"null forest" in lib.gpbc_last_error(), k
        assert lib.gpbc_fr_forest_weights(None, p, p, SZ(k), o, q) == -1 and b"null forest" in lib.gpbc_last_error(), k
        assert lib.gpbc_fr_forest_weights_dev(None, p, p, SZ(k), o, q, None) == -1 and b"null forest" in lib.gpbc_last_error(), k
    assert not out.any() and not ok.any() and not buf.any()
    assert lib.gpbc_share_forest_destroy(None) == 0
    assert [fn(None) for fn in (lib.gpbc_share_forest_trees, lib.gpbc_share_forest_leaves, lib.gpbc_share_forest_coeffs)] == [0, 0, 0]
    assert lib.gpbc_share_forest_tree_leaves(None, 0) == 0 and lib.gpbc_share_forest_tree_coeffs(None, 0) == 0


def test_wrapper_rejects_malformed_arguments():
    """ValueError before any C call.  ShareForest() itself needs a device; the checks of share() and weights() run on an object that has
    the fields they read and no handle, and every call must fail before it gets as far as asking for one."""
    import torch
    from gopairingbasedcryptography_amd import bn254
    f = object.__new__(bn254.ShareForest)
    f.trees, f.leaves, f.coeffs, f._h = 2, 3, 2, ctypes.c_void_p()
    z = lambda n: np.zeros(n, dtype=np.uint8)
    ids, buf = np.zeros(2, dtype=np.uint32), z(16 * 32)
    bad = [
        (lambda: f.weights(ids, z(5)), "expected 2 x 3"),
        (lambda: f.weights(ids, [[1, 0], [1, 0]]), "every item needs 3"),
        (lambda: f.weights(ids, np.zeros(6, dtype=np.float32)), "uint8 or bool"),
        (lambda: f.weights(np.zeros(2, dtype=np.int64), z(6)), "tree_of must be uint32"),
        (lambda: f.weights([0, -1], z(6)), "unsigned 32-bit"),
        (lambda: f.weights(torch.zeros(2, dtype=torch.int64), z(6)), "int32 tensor"),
        (lambda: f.weights(ids, z(6), out=torch.zeros(2 * 3 * 32, dtype=torch.uint8)), "all be CUDA tensors or all host"),
        (lambda: f.weights(ids, z(6), out=z(3 * 32)), "out must be"),
        (lambda: f.weights(ids, z(6), ok_out=z(3)), "ok_out must be"),
        (lambda: f.weights(ids, buf[:6], out=buf[:2 * 3 * 32]), "overlaps"),
        (lambda: f.weights(ids, z(6), out=buf[:2 * 3 * 32], ok_out=buf[32:34]), "overlaps"),
        (lambda: f.weights(ids, z(6)), "closed"),
        (lambda: f.share(ids, [1, 2, 3], z(4 * 32)), "3 scalars for 2 tree ids"),
        (lambda: f.share(ids, [1, 2]), "needs 2 coefficients"),
        (lambda: f.share(ids, [1, 2], z(3 * 32)), "expected 2 x 2"),
        (lambda: f.share(ids, [1, 2], buf[:4 * 32], out=buf[64:64 + 2 * 3 * 32]), "overlaps"),
        (lambda: f.share(ids, [1, 2], z(4 * 32), out=z(32)), "out must be"),
        (lambda: f.share(ids, [1, 2], z(4 * 32)), "closed"),
    ]
    for call, why in bad:
        with pytest.raises(ValueError, match=why):
            call()
    w, ok = f.weights(np.zeros(0, dtype=np.uint32), z(0))                                    # no items: nothing to do, no handle asked for
    assert w.shape == (0, 3, 32) and ok.shape == (0,)
    out, ok = f.share([], [], z(0))
    assert out.shape == (0, 3, 32) and ok.shape == (0,)
    for lists, why in (([], "at least one tree"), ([[(sc.ROOT_MARK, 0)], [(0, 1), (0, 0)]], "malformed tree 1: node 0"), ([[(sc.ROOT_MARK, 0)], "x"], "tree 1: nodes must be")):
        with pytest.raises(ValueError, match=why):
            bn254.ShareForest(lists)


def test_no_cpu_fallback_for_forests(lib):
    """without a GPU there is no handle to be had, and nothing computes shares or weights in its place"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gopairingbasedcryptography_amd import bn254, EngineError
    with pytest.raises(EngineError):
        bn254.ShareForest([GOOD, [(sc.ROOT_MARK, 0)]])
    nodes, off = forest_of([GOOD, GOOD])
    h = VP(1)
    assert lib.gpbc_share_forest_create(VP(nodes.ctypes.data), VP(off.ctypes.data), SZ(2), ctypes.byref(h)) < 0 and h.value is None and lib.gpbc_last_error()
