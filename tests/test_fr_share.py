"""Secret sharing in Fr (csrc/share29.hip.hpp; csrc/gpbc_fr.hip: k_fr_poly_eval, k_fr_share_tree; include/gpbc_bn254_share.h), CPU part.

Both kernels as they are launched — geometry, staging into a checked stand-in for the LDS block, lane mapping, level by level and
workgroup by workgroup — compiled for the host with -DGPBC_BOUNDS (tools/bounds_check.cpp: hc_fr_poly_eval, hc_fr_share_tree), against
the Python-integer restatement of tests/share_cases.py on every case, exactly.  Every product in that build asserts its int64 columns
for ANY input of its interval class and every canonical form its input range, so a run that finishes is the overflow proof.  Then the
new header against _lib.SHARE_SIGNATURES, the build's dependency lists, and the argument checks that need no device."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from bounds_harness import hc  # noqa: F401  (the fixture)
import abi_headers
import fr_cases as fc
import share_cases as sc
from gopairingbasedcryptography_amd import bsw07

VP, SZ = ctypes.c_void_p, ctypes.c_size_t
R = fc.R


def hc_poly(hc, geoms=None):
    def call(c, nc, d, p, npts, m, k):
        out = np.full((k * m + 1, 32), 0xA5, dtype=np.uint8)
        geom = np.zeros(5, dtype=np.uint32)
        assert hc.hc_fr_poly_eval(c.ctypes.data, nc, d, p.ctypes.data, npts, m, k, out.ctypes.data, geom.ctypes.data) == 0
        assert (out[k * m] == 0xA5).all() and geom[4] == k * m                       # every output's lane ran exactly once
        if geoms is not None:
            geoms.append(tuple(int(v) for v in geom[:4]))
        return out[:k * m]
    return call


def hc_tree(hc, geoms=None):
    def call(nodes, secrets, coeffs, k):
        L = int((nodes[:, 1] == 0).sum())
        out = np.full((k * L + 1, 32), 0xA5, dtype=np.uint8)
        geom = np.zeros(7, dtype=np.uint32)
        assert hc.hc_fr_share_tree(nodes.ctypes.data, len(nodes), secrets.ctypes.data, None if coeffs is None else coeffs.ctypes.data, k, out.ctypes.data, geom.ctypes.data) == 0
        assert (out[k * L] == 0xA5).all() and geom[0] == L
        if geoms is not None:
            geoms.append(tuple(int(v) for v in geom))
        return out[:k * L]
    return call


# ------------------------------------------------------------------------------------------------ the restatement and the case lists
def test_restatement_reconstructs_every_gate():
    """for every gate of every case any `threshold` children combine through bsw07.lagrange_at_zero to the gate's value, and the root's
    value is the secret (the first threshold children, the last, and a strided choice)"""
    n = 0
    for c in sc.tree_cases():
        for s, q in list(zip(c["secrets"], c["coeffs"]))[:2]:
            gates = []
            sc.share(c["tree"], s, q, gates)
            if gates:
                assert gates[0][1] == s % R, c["label"]
            for t, value, vals in gates[:40]:
                nch = len(vals)
                for idx in {tuple(range(1, t + 1)), tuple(range(nch - t + 1, nch + 1)), tuple(sorted(range(1, nch + 1), key=lambda i: (i * 7) % nch)[:t])}:
                    if t > 300 and idx[0] != 1:
                        continue                                                        # a 1024-point interpolation in Python integers, once
                    assert sum(bsw07.lagrange_at_zero(i, idx) * vals[i - 1] for i in idx) % R == value, (c["label"], t)
                    n += 1
    assert n > 100


def test_restatement_is_the_fixture_recursion():
    """sc.share with the fixture's "poly%d" stream in its draw order gives tests/bsw07_fixture.share_secret's shares"""
    import bsw07_fixture as bf
    tree = bf.example_tree()
    bsw07.assign_leaf_ids(tree)
    want = {}
    bf.share_secret(tree, 12345, want, tag="poly7", counter=[0])
    q = [bf.sc("poly7", i + 1) for i in range(sc.n_coeffs(tree))]
    assert sc.share(tree, 12345, q) == [want[i] for i in sorted(want)]


def test_case_lists_cover_what_they_claim():
    poly = sc.poly_cases() + [sc.poly_big_case()]
    assert {c["d"] for c in poly} >= set(sc.POLY_D) and {c["m"] for c in poly} >= set(sc.POLY_M) and {c["k"] for c in poly} >= {1, 3, 65}
    assert {(len(c["coeffs"]), len(c["points"])) for c in sc.poly_row_cases()} == {(1, 1), (1, 3), (3, 1), (3, 3)}
    vals = sc.poly_value_cases()
    assert {0, 1, R - 1, R, sc.TOP} <= set(vals[0]["points"][0]) and any(not any(c["coeffs"][0]) for c in vals) and any(c["coeffs"][0][-1] == 0 and any(c["coeffs"][0]) for c in vals)
    trees = {c["label"]: c for c in sc.tree_cases()}
    for n in (2, 3, 64, 65, 256):
        assert "%d-of-%d" % (n, n) in trees
    assert {"leaf", "1-of-1", "1-of-5", "1-of-1024", "1024-of-1024", "example", "chain8", "16x16", "alternating"} <= set(trees)
    assert {c["k"] for c in trees.values()} >= {1, 2, 65, 130}
    assert {0, R - 1} <= {s for c in trees.values() for s in c["secrets"]} and any(s >= R for c in trees.values() for s in c["secrets"])
    assert len(sc.preorder(sc.chain(8))) == 8 + 5 and sc.n_coeffs(sc.sixteen_by_sixteen()) == 17 * 15


# ------------------------------------------------------------------------------------------------ the kernels under bounds
def test_poly_eval_cases_as_launched(hc):
    assert sc.run_poly_cases(hc_poly(hc), sc.poly_cases()) == []


def test_poly_eval_1024_by_1024_as_launched(hc):
    geoms = []
    assert sc.run_poly_cases(hc_poly(hc, geoms), [sc.poly_big_case()]) == []
    assert geoms == [(1, 16, 1, 16)]


def test_poly_eval_geometry(hc):
    """(rows per workgroup, workgroups per row, LDS instance, workgroups) of the shapes that take each path"""
    shapes = [(16, 24, 65, 65), (3, 64, 1, 1), (64, 1, 65, 65), (65, 1, 65, 65), (256, 257, 1, 1), (257, 64, 3, 3), (1024, 1, 3, 3), (5, 7, 3, 1), (300, 2, 5, 5)]
    geoms = []
    for d, m, k, nc in shapes:
        c = sc._poly("geom-%d-%d-%d-%d" % (d, m, k, nc), d, m, k, nc)
        assert sc.run_poly_cases(hc_poly(hc, geoms), [c]) == []
    assert geoms == [(2, 1, 0, 33), (1, 1, 0, 1), (16, 1, 1, 5), (15, 1, 1, 5), (1, 5, 0, 5), (1, 1, 1, 3), (1, 1, 1, 3), (9, 1, 0, 1), (3, 1, 1, 2)]


def test_tree_cases_as_launched(hc):
    geoms = []
    cases = sc.tree_cases()
    assert sc.run_tree_cases(hc_tree(hc, geoms), cases) == []
    by = {c["label"]: g for c, g in zip(cases, geoms)}
    # [L, G, C, depth, items per workgroup, LDS instance, workgroups]
    assert by["leaf"] == (1, 0, 0, 0, 64, 0, 2) and by["1-of-5"] == (5, 1, 0, 1, 12, 0, 6)
    assert by["256-of-256"] == (256, 1, 255, 1, 1, 0, 2) and by["1024-of-1024"] == (1024, 1, 1023, 1, 1, 1, 1)
    assert by["16x16"] == (256, 17, 255, 2, 1, 0, 2) and by["chain8"] == (5, 8, 4, 8, 22, 0, 3)
    assert by["example"][:4] == (6, 3, 2, 2) and by["example"][4] == 16


def test_bound_margins_after_sharing(hc):
    st = np.zeros(7)
    sc.run_poly_cases(hc_poly(hc), sc.poly_value_cases())
    hc.hc_stats(st.ctypes.data_as(VP))
    assert 0 < st[0] < 2.0**63 and st[1] < 2.0**31 and st[2] < 128


def test_harness_refuses_malformed_trees_and_arguments(hc):
    z = np.zeros(64 * 32, dtype=np.uint8)
    p = z.ctypes.data
    for args in ((p, 1, 0, p, 1, 1, 1), (p, 1, 1025, p, 1, 1, 1), (p, 1, 1, p, 1, 0, 1), (p, 1, 1, p, 1, 1025, 1), (p, 2, 1, p, 1, 1, 3), (p, 1, 1, p, 2, 1, 3), (p, 1, 1, p, 1, 1, 0)):
        assert hc.hc_fr_poly_eval(*args, p, None) == -1, args
    why = ctypes.create_string_buffer(96)
    for name, nodes in sc.MALFORMED.items():
        a = sc.node_array(nodes)
        assert hc.hc_fr_share_plan(a.ctypes.data if len(a) else None, len(a), None, why) == -1 and why.value, name
        assert hc.hc_fr_share_tree(a.ctypes.data if len(a) else None, len(a), p, p, 1, p, None) == -1, name
    sizes = np.zeros(6, dtype=np.uint32)
    a = sc.node_array(sc.preorder(sc.sixteen_by_sixteen()))
    assert hc.hc_fr_share_plan(a.ctypes.data, len(a), sizes.ctypes.data, why) == 0 and sizes.tolist() == [256, 17, 255, 2, 16, 272]


# ------------------------------------------------------------------------------------------------ the header, the table, the build
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


def test_share_signature_table_is_the_share_header(lib):
    from gopairingbasedcryptography_amd import _lib
    protos = abi_headers.prototypes("gpbc_bn254_share.h")
    assert sorted(protos) == sorted(_lib.SHARE_SIGNATURES) and len(protos) == 9
    ctype = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int}
    for name, (ret, params) in protos.items():
        assert _lib.SHARE_SIGNATURES[name] == ret + ":" + "".join(params), name
        fn = getattr(lib, name)
        assert fn.restype is ctype[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [ctype[k] for k in params], name
    assert lib.gpbc_share_version() == 1 and lib.gpbc_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "gpbc_bn254_share.h")).read()
    assert '#include "gpbc_bn254.h"' in header and "1024 leaves" in header and "1024 gates" in header and "1024 children" in header


def test_build_lists_cover_the_new_header_and_lane_functions():
    from gopairingbasedcryptography_amd import _build
    assert "share29.hip.hpp" in _build.HEADERS
    assert 'include "share29.hip.hpp"' in open(os.path.join(_build.CSRC, "gpbc_fr.hip")).read()


# ------------------------------------------------------------------------------------------------ arguments, without a device
def test_wrappers_reject_malformed_arguments():
    """ValueError before any C call (no device is touched: this runs without a GPU)"""
    import torch
    from gopairingbasedcryptography_amd import bn254
    z = lambda n: np.zeros(n, dtype=np.uint8)
    t = lambda n: torch.zeros(n, dtype=torch.uint8)
    f = bn254.fr_poly_eval
    buf = z(12 * 32)
    bad = [
        lambda: f(z(4 * 32), z(32), m=1),                            # bytes without d
        lambda: f(z(4 * 32), z(32), 2),                              # bytes without m
        lambda: f(z(4 * 32), z(32), 0, 1),
        lambda: f(z(1025 * 32), z(32), 1025, 1),
        lambda: f(z(32), z(1025 * 32), 1, 1025),
        lambda: f(z(5 * 32), z(32), 2, 1),                           # not whole rows
        lambda: f(z(33), z(32), 1, 1),
        lambda: f([[1, 2], [3]], [[1]]),                             # ragged
        lambda: f([[1 << 256, 2]], [[1]]),                           # not a 32-byte value
        lambda: f(z(6 * 32), z(2 * 32), 2, 1),                       # 3 coefficient rows, 2 point rows
        lambda: f(np.zeros(64, dtype=np.int8), z(32), 2, 1),         # dtype
        lambda: f(z(64), t(32), 2, 1),                               # host / device mix
        lambda: f(t(64), t(32), 2, 1),                               # host tensors: not CUDA
        lambda: f(z(6 * 32), z(32), 2, 1, out=z(2 * 32)),            # out too small (3 rows x 1)
        lambda: f(z(6 * 32), z(32), 2, 1, out=np.zeros(3 * 32, dtype=np.int8)),
        lambda: f(buf[:6 * 32], z(32), 2, 1, out=buf[5 * 32:8 * 32]),   # out overlaps coeffs
        lambda: f(z(64), buf[:3 * 32], 2, 3, out=buf[2 * 32:5 * 32]),   # out overlaps points
    ]
    for name, nodes in sc.MALFORMED.items():
        bad.append(lambda nodes=nodes: bn254.ShareTree(nodes))
    bad += [lambda: bn254.ShareTree([(1, 2, 3)]), lambda: bn254.ShareTree([(-1, 0)]), lambda: bn254.ShareTree([(1 << 32, 0)])]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    assert f(z(0), z(0), 2, 3).shape == (0, 3, 32)                   # no rows: nothing to do, no device needed
    for name, nodes in sc.MALFORMED.items():
        assert bn254.share_tree_check(nodes), name
    for c in sc.tree_cases():
        assert bn254.share_tree_check(sc.preorder(c["tree"])) is None, c["label"]


def test_c_entries_reject_invalid_arguments(lib):
    """GPBC_ERR_INVALID_ARG with a message, nothing written, before any device is touched; k = 0 is a no-op"""
    buf, out = np.zeros(64 * 32, np.uint8), np.zeros(64 * 32, np.uint8)
    p, o = VP(buf.ctypes.data), VP(out.ctypes.data)
    host, dev = lib.gpbc_fr_poly_eval, lib.gpbc_fr_poly_eval_dev
    bad = [
        (p, 1, 0, p, 1, 1, 1, o, b"d and m"), (p, 1, 1025, p, 1, 1, 1, o, b"d and m"), (p, 1, 1, p, 1, 0, 1, o, b"d and m"), (p, 1, 1, p, 1, 1025, 1, o, b"d and m"),
        (p, 1, 0, p, 1, 1, 0, o, b"d and m"),                                            # an invalid shape is refused whatever k
        (p, 2, 4, p, 1, 4, 3, o, b"n_coeff_rows"), (p, 0, 4, p, 1, 4, 3, o, b"n_coeff_rows"), (p, 1, 4, p, 2, 4, 3, o, b"n_point_rows"), (p, 3, 4, p, 0, 4, 3, o, b"n_point_rows"),
        (None, 1, 4, p, 1, 4, 1, o, b"null"), (p, 1, 4, None, 1, 4, 1, o, b"null"), (p, 1, 4, p, 1, 4, 1, None, b"null"),
        (p, 1, 4, p, 1, 4, 1 << 29, o, b"too many rows"), (p, 1, 4, p, 1, 4, (1 << 64) - 1, o, b"too many rows"),
        (p, 1, 4, o, 1, 4, 2, p, b"overlaps"), (p, 3, 4, o, 1, 4, 3, VP(buf.ctypes.data + 11 * 32), b"overlaps"), (o, 1, 4, p, 2, 4, 2, VP(buf.ctypes.data + 7 * 32), b"overlaps"),
    ]
    for a in bad:
        for fn, extra in ((host, []), (dev, [None])):
            rc = fn(a[0], SZ(a[1]), SZ(a[2]), a[3], SZ(a[4]), SZ(a[5]), SZ(a[6]), a[7], *extra)
            assert rc == -1 and a[8] in lib.gpbc_last_error(), (a[1:7], lib.gpbc_last_error())
    assert host(None, SZ(1), SZ(4), None, SZ(1), SZ(4), SZ(0), None) == 0 and dev(None, SZ(1), SZ(4), None, SZ(1), SZ(4), SZ(0), None, None) == 0
    # trees: every malformed list is refused before the device is touched, with *out = NULL
    for name, nodes in sc.MALFORMED.items():
        a = sc.node_array(nodes)
        h = VP(1)
        assert lib.gpbc_share_tree_create(VP(a.ctypes.data) if len(a) else None, SZ(len(a)), ctypes.byref(h)) == -1 and b"malformed tree" in lib.gpbc_last_error(), name
        assert h.value is None, name
    a = sc.node_array([(sc.ROOT_MARK, 0)])
    assert lib.gpbc_share_tree_create(VP(a.ctypes.data), SZ(1), None) == -1 and b"null" in lib.gpbc_last_error()
    assert lib.gpbc_share_tree_leaves(None) == 0 and lib.gpbc_share_tree_coeffs(None) == 0 and lib.gpbc_share_tree_destroy(None) == 0
    for fn, extra in ((lib.gpbc_fr_share_tree, []), (lib.gpbc_fr_share_tree_dev, [None])):
        assert fn(None, p, p, SZ(1), o, *extra) == -1 and b"null tree" in lib.gpbc_last_error()
        assert fn(None, p, p, SZ(0), o, *extra) == -1                                   # ... also for no items: there is no tree to ask
    assert not out.any() and not buf.any()


def test_no_cpu_fallback_for_sharing(lib):
    """without a GPU a valid call returns a negative status, writes nothing and leaves a message"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gopairingbasedcryptography_amd import bn254, EngineError
    out = np.zeros((1, 3, 32), np.uint8)
    with pytest.raises(EngineError):
        bn254.fr_poly_eval([[1, 2, 3]], [[4, 5, 6]], out=out)
    with pytest.raises(EngineError):
        bn254.ShareTree([(bn254.SHARE_ROOT, 0)])
    c = fc.rows([1, 2, 3])
    p = lambda a: VP(a.ctypes.data)
    assert lib.gpbc_fr_poly_eval(p(c), SZ(1), SZ(3), p(c), SZ(1), SZ(3), SZ(1), p(out)) < 0 and lib.gpbc_last_error()
    assert lib.gpbc_fr_poly_eval_dev(p(c), SZ(1), SZ(3), p(c), SZ(1), SZ(3), SZ(1), p(out), None) < 0
    assert not out.any()
