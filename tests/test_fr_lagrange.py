"""The Lagrange basis kernel (csrc/fr29.hip.hpp: fr_lagrange_lane; csrc/gpbc_fr.hip: k_fr_lagrange_basis), CPU part.

The lane function of the kernel, compiled for the host with -DGPBC_BOUNDS (tools/bounds_check.cpp: hc_fr_lagrange_basis), against
Python's integers modulo r, exactly: the sizes, shapes, edge values and broadcast forms of tests/fr_lagrange_cases.py, B = m = 1024,
the interpolation identity and the computeT node list.  Every product in that build asserts its int64 columns and every canonical
form its input range, so a run that finishes is the overflow proof.  Then the wrapper's argument checks, the C entries' and the
missing CPU fallback."""
import ctypes

import numpy as np
import pytest

from bounds_harness import hc  # noqa: F401  (the fixture)
import fr_cases as fc
import fr_lagrange_cases as lc

VP, SZ = ctypes.c_void_p, ctypes.c_size_t
R = fc.R


def hc_call(hc, g=0):
    def call(s, ns, B, nd, nn, m, x, nx, k):
        out = np.full((k * m + 1, 32), 0xA5, dtype=np.uint8)
        p = lambda a: None if a is None else a.ctypes.data
        assert hc.hc_fr_lagrange_basis(p(s), ns, B, p(nd), nn, m, p(x), nx, k, out.ctypes.data, g) == 0
        assert (out[k * m] == 0xA5).all()
        return out[:k * m]
    return call


def hc_launch(hc, geoms=None):
    """the kernel as it is launched: geometry, staging into a checked stand-in for the LDS block, lane mapping, workgroup by workgroup"""
    def call(s, ns, B, nd, nn, m, x, nx, k):
        out = np.full((k * m + 1, 32), 0xA5, dtype=np.uint8)
        geom = np.zeros(6, dtype=np.uint32)
        p = lambda a: None if a is None else a.ctypes.data
        assert hc.hc_fr_lagrange_launch(p(s), ns, B, p(nd), nn, m, p(x), nx, k, out.ctypes.data, geom.ctypes.data) == 0
        assert (out[k * m] == 0xA5).all() and geom[5] == k * geom[0]          # every row's lanes ran exactly once
        if geoms is not None:
            geoms.append(tuple(int(v) for v in geom[:5]))
        return out[:k * m]
    return call


def test_python_expectation_is_the_reference_loop():
    """one inversion per output and the reference's factor-by-factor loop agree (B <= 17), so `basis` may stand for it everywhere"""
    n = 0
    for c in lc.all_cases():
        if c["B"] > 17:
            continue
        for j in range(c["k"]):
            S = c["set"][j if len(c["set"]) > 1 else 0]
            N = S if c["nodes"] is None else c["nodes"][j if len(c["nodes"]) > 1 else 0]
            x = 0 if c["x"] is None else c["x"][j if len(c["x"]) > 1 else 0]
            for t in N:
                assert lc.basis(S, t, x) == lc.basis_reference_loop(S, t, x), c["label"]
                n += 1
    assert n > 3000


def test_case_lists_cover_what_they_claim(hc):
    G = hc.hc_fr_lagrange_g()
    assert G == lc.G == 4
    sizes = lc.size_cases()
    assert {c["B"] for c in sizes} == set(lc.SIZES_B)
    assert {c["k"] * c["m"] for c in sizes} >= {1, G - 1, G + 1, 63, 65, 1000}
    combos = {(len(c["set"]), len(c["nodes"]) if c["nodes"] else 0, len(c["x"]) if c["x"] else 0) for c in lc.broadcast_cases()}
    assert combos == {(a, b, c) for a in (1, 5) for b in (0, 1, 5) for c in (0, 1, 5)}


def test_cases_under_bounds(hc):
    assert lc.run_cases(hc_call(hc), lc.all_cases()) == []


def test_cases_as_launched(hc):
    """every case and B = m = 1024 through the launch geometry of the kernel: no store or load outside a workgroup's staged sets, every
    output written once, Python's values; and the shapes of fr_lagrange_cases.geometry_cases take the paths they are there for
    (gpr, rows per workgroup, workgroups per row, the 1024-element LDS form, workgroups)"""
    assert lc.run_cases(hc_launch(hc), lc.all_cases() + [lc.big_case()]) == []
    geoms = []
    assert lc.run_cases(hc_launch(hc, geoms), lc.geometry_cases()) == []
    assert geoms == [(4, 16, 1, 0, 3), (2, 32, 1, 1, 3), (1, 15, 1, 1, 5), (75, 1, 2, 1, 6), (5, 12, 1, 0, 11), (2, 32, 1, 1, 4)]
    geoms = []
    lc.run_cases(hc_launch(hc, geoms), [lc.big_case()])
    assert geoms == [(256, 1, 4, 1, 8)]


def test_one_output_per_lane_gives_the_same(hc):
    """the group size is not part of the result: G = 1 (an inversion per output) on the value and broadcast lists"""
    assert lc.run_cases(hc_call(hc, g=1), lc.value_cases() + lc.broadcast_cases()) == []


def test_b_1024_under_bounds(hc):
    c = lc.big_case()
    assert lc.run_cases(hc_call(hc), [c]) == []
    assert lc.expected(c)[1024 + 777] == 1 and sum(lc.expected(c)[1024:]) == 1      # x inside its set: an indicator row


def test_values_spelled_out(hc):
    """the semantics of the header, one by one, on numbers small enough to read"""
    call = hc_call(hc)
    one = lambda S, N, x: fc.ints(call(fc.rows(S), 1, len(S), None if N is None else fc.rows(N), 1 if N else 0, len(N or S), None if x is None else fc.rows([x]), 0 if x is None else 1, 1))
    inv = lambda a: pow(a, -1, R)
    assert one([1, 2], None, None) == [2, R - 1]                                       # Delta_1(0) = (0 - 2) / (1 - 2), Delta_2(0) = (0 - 1) / (2 - 1)
    assert one([1, R + 1], None, 5) == [1, 1]                                          # equal by value: both skipped, the empty product
    assert one([0, 5 * R, 3], None, 7) == [4 * inv(R - 3) % R] * 2 + [49 * inv(9) % R]
    assert one([4, 4, 6], [6], 5) == [inv(4)]                                 # (5 - 4)^2 / (6 - 4)^2: one factor per occurrence
    assert one([4, 6], [9], 4) == [0]                                                  # x equal to a set element other than the node
    assert one([4, 6], [4], 4) == [1]
    assert one([3], [(1 << 256) - 1], (1 << 256) - 2) == [((1 << 256) - 5) * inv((1 << 256) - 4) % R]
    z = lc.rand_rows("zz", 3, 7)
    omitted = call(lc.flat(z), 3, 7, None, 0, 7, None, 0, 3)
    zeros = call(lc.flat(z), 3, 7, None, 0, 7, fc.rows([0, R, 5 * R]), 3, 3)
    assert (omitted == zeros).all()


@pytest.mark.parametrize("B", [1, 2, 5, 16, 33])
def test_interpolation_identity(hc, B):
    """for distinct nodes sum_i Delta_i(x) q(s_i) = q(x) for a random q of degree B - 1, at x outside and inside the set"""
    S = fc.rand("int-s-%d" % B, B)
    q = fc.rand("int-q-%d" % B, B)
    ev = lambda x: sum(c * pow(x, i, R) for i, c in enumerate(q)) % R
    xs = fc.rand("int-x-%d" % B, 3) + [S[B // 2], 0]
    got = fc.ints(hc_call(hc)(fc.rows(S), 1, B, None, 0, B, fc.rows(xs), len(xs), len(xs)))
    for j, x in enumerate(xs):
        assert sum(d * ev(s) for d, s in zip(got[j * B:(j + 1) * B], S)) % R == ev(x), (B, j)


@pytest.mark.parametrize("n", [1, 16])
def test_compute_t_node_list(hc, n):
    """computeT's call shape: the set N = {1 .. n+1}, the nodes 0 .. n (the loop index is the node: node 0 is outside the set and
    keeps all n + 1 factors).  For x in N the basis is 0 at node 0 and an indicator on the rest."""
    N, nodes = list(range(1, n + 2)), list(range(n + 1))
    xs = fc.rand("ct-%d" % n, 4) + N + [0, R + 2]
    got = fc.ints(hc_call(hc)(fc.rows(N), 1, n + 1, fc.rows(nodes), 1, n + 1, fc.rows(xs), len(xs), len(xs)))
    for j, x in enumerate(xs):
        row = got[j * (n + 1):(j + 1) * (n + 1)]
        assert row == [lc.basis(N, t, x) for t in nodes]
        if x % R in N:
            assert row == [0] + [1 if t == x % R else 0 for t in nodes[1:]], x
    j = 4 + n                                                                           # x = n + 1: in the set, not among the nodes
    assert got[j * (n + 1):(j + 1) * (n + 1)] == [0] * (n + 1)
    j = len(xs) - 2                                                                     # x = 0 = node 0: 1 there; the others are Delta_t over N + {0} without the factor of 0
    assert got[j * (n + 1)] == 1


def test_bound_margins_after_lagrange(hc):
    st = np.zeros(7)
    lc.run_cases(hc_call(hc), lc.value_cases())
    hc.hc_stats(st.ctypes.data_as(VP))
    assert 0 < st[0] < 2.0**63 and st[1] < 2.0**31 and st[2] < 128


def test_harness_arguments(hc):
    z = np.zeros(64 * 32, dtype=np.uint8)
    p = z.ctypes.data
    for args in ((p, 1, 0, None, 0, 0, None, 0, 1), (p, 1, 1025, None, 0, 1025, None, 0, 1), (p, 1, 4, None, 0, 5, None, 0, 1), (p, 2, 4, None, 0, 4, None, 0, 3),
                 (p, 1, 4, p, 2, 4, None, 0, 3), (p, 1, 4, None, 0, 4, p, 2, 3), (p, 1, 4, None, 0, 4, None, 1, 3), (p, 1, 4, p, 1, 0, None, 0, 1)):
        assert hc.hc_fr_lagrange_basis(*args, p, 0) == -1, args
    assert hc.hc_fr_lagrange_basis(p, 1, 4, None, 0, 4, None, 0, 1, p, 3) == -1          # a group size the harness does not instantiate


# ------------------------------------------------------------------------------------------------ the wrapper and the C entries
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


def test_abi_version_counts_the_entry(lib):
    assert lib.gpbc_abi_version() == 8


def test_wrapper_rejects_malformed_arguments():
    """ValueError before any C call (no device is touched: this runs without a GPU)"""
    import torch
    from gopairingbasedcryptography_amd import bn254
    z = lambda n: np.zeros(n, dtype=np.uint8)
    t = lambda n: torch.zeros(n, dtype=torch.uint8)
    f = bn254.fr_lagrange_basis
    bad = [
        lambda: f(z(4 * 32)),                                        # bytes without B
        lambda: f(z(4 * 32), 0),
        lambda: f(z(1025 * 32), 1025),
        lambda: f(z(5 * 32), 2),                                     # not whole rows
        lambda: f(z(33), 1),
        lambda: f([[1, 2], [3]]),                                    # ragged
        lambda: f([[1, 2]], 3),                                      # B against the rows
        lambda: f([[1 << 256, 2]]),                                  # not a 32-byte value
        lambda: f([[1, 2]], m=3),                                    # without nodes m is B
        lambda: f(z(4 * 32), 2, nodes=z(3 * 32)),                    # nodes without m
        lambda: f(z(4 * 32), 2, nodes=z(3 * 32), m=2),
        lambda: f(z(4 * 32), 2, nodes=z(2 * 32), m=1025),
        lambda: f(z(6 * 32), 2, nodes=z(4 * 32), m=2),               # 3 set rows, 2 node rows
        lambda: f(z(6 * 32), 2, x=z(2 * 32)),                        # 3 rows, 2 x
        lambda: f(z(6 * 32), 2, x=z(33)),
        lambda: f(z(2 * 32), 2, nodes=z(3 * 2 * 32), m=2, x=[1, 2]),  # 3 node rows, 2 x
        lambda: f(np.zeros(64, dtype=np.int8), 2),                   # dtype
        lambda: f(z(64), 2, x=t(32)),                                # host / device mix
        lambda: f(t(64), 2, nodes=z(64), m=2),
        lambda: f(t(64), 2),                                         # right sizes, but host tensors: not CUDA
        lambda: f(t(64).to(torch.int8), 2),
        lambda: f(z(6 * 32), 2, out=z(5 * 32)),                      # out too small (3 rows x 2)
        lambda: f(z(6 * 32), 2, out=np.zeros(6 * 32, dtype=np.int8)),
        lambda: f(z(2 * 32), 2, nodes=z(3 * 32), m=3, out=z(2 * 32)),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    assert f(z(0), 2).shape == (0, 2, 32)                            # no rows: nothing to do, no device needed


def test_c_entries_reject_invalid_arguments(lib):
    """GPBC_ERR_INVALID_ARG with a message, nothing written, before any device is touched; k = 0 is a no-op"""
    buf, out = np.zeros(64 * 32, np.uint8), np.zeros(64 * 32, np.uint8)
    p, o = VP(buf.ctypes.data), VP(out.ctypes.data)
    S = lambda *a: [SZ(v) for v in a]
    host, dev = lib.gpbc_fr_lagrange_basis, lib.gpbc_fr_lagrange_basis_dev
    bad = [
        (p, 1, 0, None, 0, 0, None, 0, 1, o, b"B and m"), (p, 1, 1025, None, 0, 1025, None, 0, 1, o, b"B and m"), (p, 1, 4, p, 1, 0, None, 0, 1, o, b"B and m"),
        (p, 1, 4, p, 1, 1025, None, 0, 1, o, b"B and m"), (p, 1, 4, None, 0, 5, None, 0, 1, o, b"m must equal B"), (p, 2, 4, None, 0, 4, None, 0, 3, o, b"n_set_rows"),
        (p, 0, 4, None, 0, 4, None, 0, 3, o, b"n_set_rows"), (p, 1, 4, p, 2, 4, None, 0, 3, o, b"n_node_rows"), (p, 1, 4, p, 0, 4, None, 0, 3, o, b"n_node_rows"),
        (p, 1, 4, None, 0, 4, p, 2, 3, o, b"nx"), (p, 1, 4, None, 0, 4, p, 0, 3, o, b"nx"), (p, 1, 4, None, 0, 4, None, 1, 3, o, b"nx"),
        (None, 1, 4, None, 0, 4, None, 0, 1, o, b"null"), (p, 1, 4, None, 0, 4, None, 0, 1, None, b"null"),
        (p, 1, 4, None, 0, 4, None, 0, 1 << 29, o, b"too many rows"), (p, 1, 4, None, 0, 4, None, 0, (1 << 64) - 1, o, b"too many rows"),
        (p, 1, 4, None, 0, 4, None, 0, 2, p, b"overlaps"), (p, 3, 4, None, 0, 4, None, 0, 3, VP(buf.ctypes.data + 11 * 32), b"overlaps"),
        (o, 1, 4, p, 1, 4, None, 0, 2, VP(buf.ctypes.data + 3 * 32), b"overlaps"), (o, 1, 4, None, 0, 4, p, 1, 2, p, b"overlaps"),
    ]
    for a in bad:
        for fn, extra in ((host, []), (dev, [None])):
            rc = fn(a[0], SZ(a[1]), SZ(a[2]), a[3], SZ(a[4]), SZ(a[5]), a[6], SZ(a[7]), SZ(a[8]), a[9], *extra)
            assert rc == -1 and a[10] in lib.gpbc_last_error(), (a[1:9], lib.gpbc_last_error())
    assert host(None, *S(1, 4), None, *S(0, 4), None, *S(0, 0), None) == 0 and dev(None, *S(1, 4), None, *S(0, 4), None, *S(0, 0), None, None) == 0
    assert not out.any() and not buf.any()


def test_no_cpu_fallback_for_lagrange(lib):
    """without a GPU a valid call returns a negative status, writes nothing and leaves a message"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gopairingbasedcryptography_amd import bn254, EngineError
    out = np.zeros((1, 3, 32), np.uint8)
    with pytest.raises(EngineError):
        bn254.fr_lagrange_basis([[1, 2, 3]], out=out)
    s = fc.rows([1, 2, 3])
    p = lambda a: VP(a.ctypes.data)
    assert lib.gpbc_fr_lagrange_basis(p(s), SZ(1), SZ(3), None, SZ(0), SZ(3), None, SZ(0), SZ(1), p(out)) < 0 and lib.gpbc_last_error()
    assert lib.gpbc_fr_lagrange_basis_dev(p(s), SZ(1), SZ(3), None, SZ(0), SZ(3), None, SZ(0), SZ(1), p(out), None) < 0
    assert not out.any()
