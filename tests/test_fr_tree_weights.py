"""Reconstruction weights of a threshold tree in Fr (csrc/recon29.hip.hpp; csrc/gpbc_fr.hip: k_fr_tree_weights; include/gpbc_bn254_recon.h),
CPU part.

The kernel as it is launched — plan, geometry, staging into a checked stand-in for the LDS block, both passes level by level and workgroup
by workgroup — compiled for the host with -DGPBC_BOUNDS (tools/bounds_check.cpp: hc_fr_tree_weights), against bsw07.decrypt_plan in Python
integers on every case of tests/tree_weight_cases.py, exactly.  Every product in that build asserts its int64 columns for ANY input of its
interval class and every canonical form its input range, so a run that finishes is the overflow proof.  Then the weights against the
shares of tests/share_cases.py, the new header against _lib.RECON_SIGNATURES, the build's dependency lists, and the argument checks that need
no device."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from bounds_harness import hc  # noqa: F401  (the fixture)
import abi_headers
import fr_cases as fc
import share_cases as sc
import tree_weight_cases as tw

VP, SZ = ctypes.c_void_p, ctypes.c_size_t
R = fc.R
GUARD = 0xA5


@pytest.fixture(scope="module")
def launched(hc):
    """{label: (w [k x L, 32], ok [k], geometry)} of every case, each run once with a guard row behind both outputs"""
    out = {}
    for c in tw.cases():
        k, L = c["k"], c["L"]
        w, ok, geom = np.full((k * L + 1, 32), GUARD, dtype=np.uint8), np.full(k + 1, GUARD, dtype=np.uint8), np.zeros(8, dtype=np.uint32)
        held = np.ascontiguousarray(c["held"])
        assert hc.hc_fr_tree_weights(c["nodes"].ctypes.data, len(c["nodes"]), held.ctypes.data, k, w.ctypes.data, ok.ctypes.data, geom.ctypes.data) == 0, c["label"]
        assert (w[k * L] == GUARD).all() and ok[k] == GUARD and geom[0] == L, c["label"]
        out[c["label"]] = (w[:k * L], ok[:k], tuple(int(v) for v in geom))
    return out


# ------------------------------------------------------------------------------------------------ the case lists
def test_case_lists_cover_what_they_claim():
    cases = tw.cases()
    labels = {c["label"].split("/")[0] for c in cases}
    assert labels == {c["label"] for c in sc.tree_cases()} | {"many-gates", "largest"}
    assert {c["k"] for c in cases} >= {1, 3, 65, 130}
    assert all(c["k"] == 1 for c in cases if c["label"].startswith(("1-of-1024", "1024-of-1024")))
    assert max(c["k"] * c["L"] for c in cases) == 130 * 256
    assert {int(v) for c in cases for v in np.unique(c["held"])} == {0, 0x01, 0x80, 0xFF}
    seen = set()
    for c in cases:
        want_w, want_ok = tw.expected(c)
        if 0 < sum(want_ok) < c["k"]:
            seen.add("satisfied and unsatisfied items in one call")
        for j, ok in enumerate(want_ok):
            row, held = want_w[j * c["L"]:(j + 1) * c["L"]], c["held"][j]
            assert all(v == 0 for v, h in zip(row, held) if not h), c["label"]
            if not ok:
                assert not any(row), c["label"]
                seen.add("unsatisfied with held leaves" if held.any() else "nothing held")
            else:
                seen.add("held leaf with weight 0" if any(h and not v for v, h in zip(row, held)) else "every held leaf used")
    assert seen == {"satisfied and unsatisfied items in one call", "unsatisfied with held leaves", "nothing held", "held leaf with weight 0", "every held leaf used"}
    # the first-k rule and a satisfied subtree behind the chosen ones, on the example tree: 2 of (11, 2 of (22, 33), 44, 1 of (55, 11))
    ex = next(c for c in cases if c["label"] == "example")
    row, ok = tw.expected_row("example", ex["tree"], ex["L"], np.ones(6, dtype=np.uint8))
    assert ok == 1 and row[0] and row[1] and row[2] and row[3:] == (0, 0, 0)


def test_expectation_is_the_lagrange_product_on_a_path():
    """3 of 5 over 2 of 3 with children 2, 4, 5 of the root satisfied through their leaves (1, 3), (2, 3), (1, 2): written out by hand"""
    from gopairingbasedcryptography_amd import bsw07
    tree, L = tw.relabel(sc.three_of_five_over_two_of_three())
    held = np.zeros(L, dtype=np.uint8)
    for child, leaves in ((2, (1, 3)), (4, (2, 3)), (5, (1, 2))):
        for x in leaves:
            held[3 * (child - 1) + x - 1] = 1
    row, ok = tw.expected_row("by-hand", tree, L, held)
    want = [0] * L
    for child, leaves in ((2, (1, 3)), (4, (2, 3)), (5, (1, 2))):
        for x in leaves:
            want[3 * (child - 1) + x - 1] = bsw07.lagrange_at_zero(child, (2, 4, 5)) * bsw07.lagrange_at_zero(x, leaves) % R
    assert ok == 1 and list(row) == want


# ------------------------------------------------------------------------------------------------ the kernel under bounds
def test_tree_weights_as_launched(launched):
    assert tw.run_cases(lambda c: launched[c["label"]][:2], tw.cases()) == []


def test_geometry_as_launched(launched):
    """[L, G, U, depth, items per workgroup, words per item, LDS instance, workgroups]"""
    g = {label: v[2] for label, v in launched.items()}
    assert g["leaf"] == (1, 0, 0, 0, 64, 1, 0, 3) and g["1-of-5"] == (5, 1, 5, 1, 52, 17, 0, 3)
    assert g["256-of-256/0"] == (256, 1, 256, 1, 4, 267, 0, 1) and g["16x16"] == (256, 17, 272, 2, 5, 443, 0, 26)
    assert g["1024-of-1024/all"] == (1024, 1, 1024, 1, 2, 1035, 0, 1) and g["chain8"][:4] == (5, 8, 12, 8)
    assert g["many-gates"] == (512, 273, 784, 3, 3, 3515, 1, 4) and g["largest/all"] == (1024, 1024, 2047, 2, 1, 12289, 1, 1)
    assert {v[6] for v in g.values()} == {0, 1}                                       # both LDS instances
    assert any(v[4] > 1 and c["k"] % v[4] and c["k"] > v[4] for c in tw.cases() for v in [g[c["label"]]])     # a last workgroup that is not full


def test_weights_recombine_the_shares(launched):
    """sum_y w_y share_y = secret for every ok = 1 item, against the ShareSecret restatement of tests/share_cases.py on the same tree"""
    shared = {c["label"]: c for c in sc.tree_cases()}
    n = 0
    for c in tw.cases():
        base = c["label"].split("/")[0]
        if base in shared:
            tree, secret, coeffs = shared[base]["tree"], shared[base]["secrets"][-1], shared[base]["coeffs"][-1]
        else:
            tree, secret, coeffs = c["tree"], sc.rand("tw-s-" + base, 1)[0], sc.rand("tw-q-" + base, sc.n_coeffs(c["tree"]))
        shares = sc.share(tree, secret, coeffs)
        w, ok, _ = launched[c["label"]]
        w = fc.ints(w)
        for j in range(c["k"]):
            if ok[j]:
                assert sum(a * b for a, b in zip(w[j * c["L"]:(j + 1) * c["L"]], shares)) % R == secret % R, (c["label"], j)
                n += 1
    assert n > 300


def test_harness_refuses_malformed_trees_and_arguments(hc):
    z = np.zeros(64 * 32, dtype=np.uint8)
    p = z.ctypes.data
    for name, nodes in sc.MALFORMED.items():
        a = sc.node_array(nodes)
        assert hc.hc_fr_tree_weights(a.ctypes.data if len(a) else None, len(a), p, 1, p, p, None) == -1, name
    a = sc.node_array([(sc.ROOT_MARK, 0)])
    for args in ((None, 1, p, p), (p, 0, p, p), (p, 1, None, p), (p, 1, p, None)):
        assert hc.hc_fr_tree_weights(a.ctypes.data, 1, args[0], args[1], args[2], args[3], None) == -1, args


# ------------------------------------------------------------------------------------------------ the header, the table, the build
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


def test_recon_signature_table_is_the_recon_header(lib):
    from gopairingbasedcryptography_amd import _lib
    protos = abi_headers.prototypes("gpbc_bn254_recon.h")
    assert sorted(protos) == sorted(_lib.RECON_SIGNATURES) == ["gpbc_fr_tree_weights", "gpbc_fr_tree_weights_dev", "gpbc_recon_version"]
    ctype = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int}
    for name, (ret, params) in protos.items():
        assert _lib.RECON_SIGNATURES[name] == ret + ":" + "".join(params), name
        fn = getattr(lib, name)
        assert fn.restype is ctype[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [ctype[k] for k in params], name
    assert lib.gpbc_recon_version() == 1 and lib.gpbc_share_version() == 1 and lib.gpbc_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "gpbc_bn254_recon.h")).read()
    assert '#include "gpbc_bn254_share.h"' in header and "Entry map" in header and "access/tree/access_tree_node.go:96-164" in header


def test_build_lists_cover_the_new_header_and_lane_functions():
    from gopairingbasedcryptography_amd import _build
    assert "recon29.hip.hpp" in _build.HEADERS
    fr = open(os.path.join(_build.CSRC, "gpbc_fr.hip")).read()
    assert 'include "recon29.hip.hpp"' in fr and "k_fr_tree_weights" in fr
    assert not os.path.exists(os.path.join(_build.CSRC, "gpbc_recon.hip"))


# ------------------------------------------------------------------------------------------------ arguments, without a device
def test_c_entries_reject_invalid_arguments(lib):
    """GPBC_ERR_INVALID_ARG with a message, nothing written, before any device is touched.  A handle needs a device, so what can be
    asked here is the null handle, whatever else is passed (tests/test_fr_tree_weights_gpu.py has the refusals of a live handle)."""
    buf, out, ok = np.zeros(64, np.uint8), np.zeros(64 * 32, np.uint8), np.zeros(64, np.uint8)
    p, o, q = VP(buf.ctypes.data), VP(out.ctypes.data), VP(ok.ctypes.data)
    for fn, extra in ((lib.gpbc_fr_tree_weights, []), (lib.gpbc_fr_tree_weights_dev, [None])):
        for k in (1, 0, 1 << 29, (1 << 64) - 1):
            assert fn(None, p, SZ(k), o, q, *extra) == -1 and b"null tree" in lib.gpbc_last_error(), k
        assert fn(None, None, SZ(1), None, None, *extra) == -1 and b"null tree" in lib.gpbc_last_error()
    assert not out.any() and not ok.any() and not buf.any()


def test_wrapper_rejects_malformed_arguments():
    """ValueError before any C call.  ShareTree() itself needs a device; the checks of weights() run on an object that has the fields they
    read and no handle, and every call must fail before it gets as far as asking for one."""
    import torch
    from gopairingbasedcryptography_amd import bn254
    t = object.__new__(bn254.ShareTree)
    t.leaves, t.coeffs, t._h = 3, 2, ctypes.c_void_p()
    z = lambda n: np.zeros(n, dtype=np.uint8)
    buf = z(16 * 32)
    bad = [
        (lambda: t.weights(z(4)), "whole items"),
        (lambda: t.weights([[1, 0]]), "every item needs 3"),                                  # a short row
        (lambda: t.weights([[1, 0, 1], [1]]), "every item needs 3"),                          # ragged
        (lambda: t.weights(np.zeros(6, dtype=np.int8)), "uint8 or bool"),
        (lambda: t.weights(np.zeros(6, dtype=np.float32)), "uint8 or bool"),
        (lambda: t.weights(torch.zeros(6, dtype=torch.int8)), "contiguous uint8 tensor"),
        (lambda: t.weights(z(6), out=torch.zeros(2 * 3 * 32, dtype=torch.uint8)), "all be CUDA tensors or all host"),
        (lambda: t.weights(z(6), out=z(3 * 32)), "out must be"),                              # too small: 2 items x 3 leaves
        (lambda: t.weights(z(6), out=np.zeros(2 * 3 * 32, dtype=np.int8)), "out must be"),
        (lambda: t.weights(z(6), ok_out=z(3)), "ok_out must be"),
        (lambda: t.weights(buf[:6], out=buf[:2 * 3 * 32]), "overlaps"),                       # out on held
        (lambda: t.weights(z(6), out=buf[:2 * 3 * 32], ok_out=buf[32:34]), "overlaps"),       # the outputs on each other
        (lambda: t.weights(buf[:6], ok_out=buf[4:6]), "overlaps"),                            # ok_out on held
        (lambda: t.weights(z(6)), "closed"),                                                  # everything in order but the tree
    ]
    for call, why in bad:
        with pytest.raises(ValueError, match=why):
            call()
    w, ok = t.weights(z(0))                                                                   # no items: nothing to do, no handle asked for
    assert w.shape == (0, 3, 32) and ok.shape == (0,)


def test_no_cpu_fallback_for_weights(lib):
    """without a GPU there is no handle to be had, and nothing computes the weights in its place"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gopairingbasedcryptography_amd import bn254, EngineError
    with pytest.raises(EngineError):
        bn254.ShareTree(sc.preorder(tw.relabel(sc.flat_gate(2, 3))[0]))
    a = sc.node_array(sc.preorder(sc.flat_gate(2, 3)))
    h = VP(1)
    assert lib.gpbc_share_tree_create(VP(a.ctypes.data), SZ(len(a)), ctypes.byref(h)) < 0 and h.value is None and lib.gpbc_last_error()


# ------------------------------------------------------------------------------------------------ node lists that are not in preorder
def test_lists_in_another_order_share_as_before_and_reconstruct(hc):
    """A list needs parent < child and no more (gpbc_share_tree_create; bn254.share_tree_check): with the children of several gates
    alternating, the sharing kernel as launched gives the shares of the restatement in list order, and the weights of every held mask are
    decrypt_plan's and recombine those shares."""
    from gopairingbasedcryptography_amd import bn254
    for name, nodes in tw.OTHER_ORDERS.items():
        assert bn254.share_tree_check(nodes) is None and sc.preorder(tw.tree_of_list(nodes)[0]) != nodes, name
        arr = sc.node_array(nodes)
        L, C = int((arr[:, 1] == 0).sum()), int(sum(t - 1 for _, t in nodes if t))
        secret, coeffs = sc.rand("tw-other-s-" + name, 1)[0], sc.rand("tw-other-q-" + name, C)
        shares = np.full((L + 1, 32), GUARD, dtype=np.uint8)
        assert hc.hc_fr_share_tree(arr.ctypes.data, len(arr), fc.rows([secret]).ctypes.data, fc.rows(coeffs).ctypes.data if C else None, 1, shares.ctypes.data, None) == 0, name
        want_shares = tw.list_share(nodes, secret, coeffs)
        assert fc.ints(shares[:L]) == want_shares and (shares[L] == GUARD).all(), name
        held = tw.all_masks(L)
        k = len(held)
        w, ok = np.full((k * L + 1, 32), GUARD, dtype=np.uint8), np.full(k + 1, GUARD, dtype=np.uint8)
        assert hc.hc_fr_tree_weights(arr.ctypes.data, len(arr), held.ctypes.data, k, w.ctypes.data, ok.ctypes.data, None) == 0, name
        assert (w[k * L] == GUARD).all() and ok[k] == GUARD, name
        got = fc.ints(w[:k * L])
        for j in range(k):
            row, want_ok = tw.list_expected(nodes, held[j])
            assert got[j * L:(j + 1) * L] == row and ok[j] == want_ok, (name, j)
            if want_ok:
                assert sum(a * b for a, b in zip(row, want_shares)) % R == secret % R, (name, j)
        assert 0 < ok[:k].sum() < k, name
