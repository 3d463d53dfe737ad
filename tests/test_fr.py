"""The scalar field Fr (csrc/fr29.hip.hpp, csrc/gpbc_fr.hip), CPU part.

The lane functions of the kernels, compiled for the host with -DGPBC_BOUNDS (tools/bounds_check.cpp: hc_fr_op,
hc_fr_poly_from_roots, hc_fr_poly_quotients), against Python's integer arithmetic modulo r, exactly: the edge values and sizes of
tests/fr_cases.py, values that are 0 modulo r at every position of an inversion group, broadcast b, in place; the two polynomial
kernels for B in {1, 2, 3, 63, 64, 65, 255, 256, 257, 1024}.  Every product in that build asserts its int64 columns and every
canonical form its input range, so a run that finishes is the overflow proof.  Then the wrapper's argument checks and the
missing CPU fallback of the C entries.

The identity "quotient for root i == product over the other roots" compares two Python functions with each other (it is what
makes afp25.quotient_by_root a valid stand-in for the reference's multiplied-out quotient); it costs B^2 / 2 big-integer steps
per root, so it runs for every root up to B = 257 and for every 64th root at B = 1024, while the device rows are compared with
quotient_by_root for every root of every B."""
import ctypes
import os

import numpy as np
import pytest

from bounds_harness import hc  # noqa: F401  (the fixture)
import fr_cases as fc
from gopairingbasedcryptography_amd import afp25

VP, SZ = ctypes.c_void_p, ctypes.c_size_t


def hc_op(hc, op, A, B=None, k=0, out=None):
    a = fc.rows(A) if not isinstance(A, np.ndarray) else A
    b = a if B is None else (fc.rows(B) if not isinstance(B, np.ndarray) else B)
    n = a.shape[0]
    out = np.zeros((n, 32), dtype=np.uint8) if out is None else out
    assert hc.hc_fr_op(fc.OP_CODE[op], a.ctypes.data, b.ctypes.data, b.shape[0], n, out.ctypes.data, k) == 0
    return out


# ------------------------------------------------------------------------------------------------ 1. elementwise
def test_elementwise_cases_under_bounds(hc):
    """every operation on the edge values (all pairs for the binary ones), random scalars in sizes 1, K - 1, K + 1, 1000, a
    broadcast b, zeros at every position of an inversion group and a group of nothing else: Python's result, bit for bit"""
    K = hc.hc_fr_inv_k()
    assert K == 8
    for label, op, A, B in fc.elementwise_cases(K):
        want = fc.rows(fc.expect(op, A, B))
        got = hc_op(hc, op, A, B)
        assert (got == want).all(), (label, op, np.nonzero((got != want).any(axis=1))[0][:8])


def test_elementwise_in_place_under_bounds(hc):
    """out = a, and out = b with one b per a: every element reads its rows before it writes its own"""
    n = 50
    A, B = fc.EDGES + fc.rand("ip-a", n), fc.rand("ip-b", n + len(fc.EDGES))
    for op in fc.BINARY + fc.UNARY:
        want = fc.rows(fc.expect(op, A, B if op in fc.BINARY else None))
        a = fc.rows(A)
        hc_op(hc, op, a, fc.rows(B) if op in fc.BINARY else None, out=a)
        assert (a == want).all(), (op, "out=a")
        if op in fc.BINARY:
            b = fc.rows(B)
            hc_op(hc, op, fc.rows(A), b, out=b)
            assert (b == want).all(), (op, "out=b")


def test_inverse_group_sizes_under_bounds(hc):
    """the shared-inversion walk for the group sizes the harness instantiates (1, 4, 8; 0 = the kernel's)"""
    A = fc.rand("gs", 37)
    A[5], A[6], A[17], A[36] = 0, fc.R, 5 * fc.R, 2 * fc.R
    want = fc.rows(fc.expect("inverse", A))
    for k in (1, 4, 8, 0):
        assert (hc_op(hc, "inverse", A, k=k) == want).all(), k
    prod = hc_op(hc, "mul", fc.ints(want), A)
    assert fc.ints(prod) == [1 if a % fc.R else 0 for a in A]


def test_mont_round_trip_is_gnark_layout(hc):
    """to_mont gives the words of fr.Element (x 2^256 mod r, canonical) and from_mont takes them back"""
    A = fc.EDGES + fc.rand("mont", 20)
    m = hc_op(hc, "to_mont", A)
    assert fc.ints(m) == [a * (1 << 256) % fc.R for a in A]
    assert fc.ints(hc_op(hc, "from_mont", fc.ints(m))) == [a % fc.R for a in A]
    assert fc.ints(hc_op(hc, "to_mont", [1]))[0] == int.from_bytes(b"".join(x.to_bytes(8, "little") for x in
                                                                             (0xac96341c4ffffffb, 0x36fc76959f60cd29, 0x666ea36f7879462e, 0x0e0a77c19a07df2f)), "little")


def fr_vector_entries(ks):
    """what tools/gnark_vectors/main.go prints under "fr" if gnark agrees with Python's integers: fr.Element words of a, b and of
    a + b, a - b, a b, -a, 1 / a for neighbouring scalars of its list"""
    word = lambda x: (x % fc.R * fc.MONT % fc.R).to_bytes(32, "little").hex()
    out = []
    for a, b in zip(ks, ks[1:]):
        a, b = int(a), int(b)
        out.append({"a": str(a), "b": str(b), "a_raw": word(a), "b_raw": word(b), "add_raw": word(a + b), "sub_raw": word(a - b), "mul_raw": word(a * b),
                    "neg_raw": word(-a), "inverse_raw": word(pow(a, -1, fc.R) if a % fc.R else 0)})
    return out


def test_fr_element_vectors(hc):
    """the consumer of the "fr" entries of tests/golden/gnark_vectors.json (tools/gnark_vectors/main.go; the file exists only once a
    maintainer with Go has run it): gnark's words go through from_mont, the operation and to_mont and must come back as gnark's words.
    The same comparison always runs over a record of that shape made from Python's integers."""
    import json
    from conftest import GOLDEN
    ks = ["1", "2", "3", "65537", "1311768467463790320", "6296462850587514219860166612309923493513421339716397012889107043265683424215", str(fc.R - 1)]
    entries = fr_vector_entries(ks)
    path = os.path.join(GOLDEN, "gnark_vectors.json")
    if os.path.exists(path):
        doc = json.load(open(path))
        entries += doc.get("fr", [])
        if "fr_inverse_of_zero_raw" in doc:
            assert doc["fr_inverse_of_zero_raw"] == "00" * 32
    assert fc.ints(hc_op(hc, "inverse", fc.ints(hc_op(hc, "from_mont", [0])))) == [0]
    raw = lambda e, key: np.frombuffer(bytes.fromhex(e[key]), dtype=np.uint8).reshape(1, 32).copy()
    for e in entries:
        a, b = hc_op(hc, "from_mont", raw(e, "a_raw")), hc_op(hc, "from_mont", raw(e, "b_raw"))
        assert fc.ints(a) == [int(e["a"]) % fc.R] and fc.ints(b) == [int(e["b"]) % fc.R]
        for op in fc.BINARY + ("neg", "inverse"):
            got = hc_op(hc, "to_mont", hc_op(hc, op, a, b if op in fc.BINARY else None))
            assert got.tobytes().hex() == e[op + "_raw"], (e["a"], e["b"], op)


def test_bound_margins_after_fr(hc):
    A = fc.rand("bm", 16)
    for op in fc.BINARY + fc.UNARY:
        hc_op(hc, op, A, A if op in fc.BINARY else None)
    st = np.zeros(7)
    hc.hc_stats(st.ctypes.data_as(VP))
    assert 0 < st[0] < 2.0**63 and st[1] < 2.0**31 and st[2] < 128


# ------------------------------------------------------------------------------------------------ 2. / 3. polynomials
def hc_from_roots(hc, polys, B):
    r = fc.rows([x for p in polys for x in p])
    out = np.zeros((len(polys), B + 1, 32), dtype=np.uint8)
    assert hc.hc_fr_poly_from_roots(r.ctypes.data, B, len(polys), out.ctypes.data) == 0
    return out


def test_x_minus_1_times_x_minus_2(hc):
    """(X - 1)(X - 2) = 2 - 3X + X^2, the reference's own example"""
    assert fc.ints(hc_from_roots(hc, [[1, 2]], 2)) == [2, fc.R - 3, 1]


@pytest.mark.parametrize("B", fc.POLY_BS)
def test_poly_from_roots_under_bounds(hc, B):
    polys = fc.poly_cases(B)
    got = hc_from_roots(hc, polys, B)
    assert fc.ints(got) == [c for p in polys for c in afp25.poly_from_roots(p)]


@pytest.mark.parametrize("B", fc.POLY_BS)
def test_poly_quotients_under_bounds(hc, B):
    """every root of every polynomial: the row is quotient_by_root's and the product over the other roots; a non-root gives ok = 0
    and a zero row while its neighbours' rows are right; strides B, B + 1, B + 7 pad with zeros"""
    polys = fc.poly_cases(B)
    coeffs, points, want = fc.quotient_case(polys, B)
    assert want[B // 2] is None and (B < 3 or want[B - 1] is None) and sum(w is None for w in want) == (2 if B >= 3 else 1)
    assert fc.others_product_matches(polys, want, B, every=64 if B > 257 else 1) is None
    c, p = fc.rows([x for f in coeffs for x in f]), fc.rows([x for q in points for x in q])
    for stride in (B, B + 1, B + 7):
        q = np.full((len(want), stride, 32), 0xA5, dtype=np.uint8)
        ok = np.full(len(want), 0xA5, dtype=np.uint8)
        assert hc.hc_fr_poly_quotients(c.ctypes.data, p.ctypes.data, B, len(polys), stride, q.ctypes.data, ok.ctypes.data) == 0
        assert fc.check_quotients(q, ok, want, B, stride) == [], (B, stride)


def test_poly_arguments_of_the_harness(hc):
    z = np.zeros(64, dtype=np.uint8)
    assert hc.hc_fr_poly_from_roots(z.ctypes.data, 0, 1, z.ctypes.data) == -1
    assert hc.hc_fr_poly_from_roots(z.ctypes.data, 1025, 1, z.ctypes.data) == -1
    assert hc.hc_fr_poly_quotients(z.ctypes.data, z.ctypes.data, 2, 1, 1, z.ctypes.data, z.ctypes.data) == -1


# ------------------------------------------------------------------------------------------------ 4. the wrapper and the C entries
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


def test_wrapper_rejects_malformed_arguments():
    """ValueError before any C call (no device is touched: this runs without a GPU)"""
    import torch
    from gopairingbasedcryptography_amd import bn254
    z = lambda n: np.zeros(n, dtype=np.uint8)
    t = lambda n: torch.zeros(n, dtype=torch.uint8)
    bad = [
        lambda: bn254.fr_add(z(5 * 32), z(3 * 32)),                              # short b
        lambda: bn254.fr_mul(z(5 * 32), z(2 * 32)),                              # nb not in {1, n}
        lambda: bn254.fr_sub([1, 2, 3], [1, 2]),
        lambda: bn254.fr_add(np.zeros(32, dtype=np.int8), z(32)),                # dtype
        lambda: bn254.fr_neg(np.zeros(8, dtype=np.uint32)),
        lambda: bn254.fr_inverse(z(33)),                                         # not whole rows
        lambda: bn254.fr_add(z(64), t(64)),                                      # host / device mix
        lambda: bn254.fr_add(t(64), z(64)),
        lambda: bn254.fr_add(t(64), t(64)),                                      # right sizes, but host tensors: not CUDA
        lambda: bn254.fr_mul(t(64).to(torch.int8), t(64).to(torch.int8)),
        lambda: bn254.fr_add(z(64), z(64), out=z(32)),                           # out too small
        lambda: bn254.fr_inverse(t(64), out=t(32)),
        lambda: bn254.fr_to_mont(z(64), out=np.zeros(64, dtype=np.int8)),
        lambda: bn254.fr_from_mont([1 << 256]),                                  # not a 32-byte value
        lambda: bn254.fr_neg([-1]),
        lambda: bn254.fr_poly_from_roots(z(0), 0),                               # B = 0
        lambda: bn254.fr_poly_from_roots(z(1025 * 32), 1025),                    # B = 1025
        lambda: bn254.fr_poly_from_roots([[1, 2], [3]]),                         # ragged
        lambda: bn254.fr_poly_from_roots(z(5 * 32), 2),                          # not a multiple of B
        lambda: bn254.fr_poly_from_roots(z(4 * 32)),                             # bytes without B
        lambda: bn254.fr_poly_from_roots(z(4 * 32), 2, out=z(5 * 32)),           # out too small (needs 2 x 3 rows)
        lambda: bn254.fr_poly_from_roots(t(4 * 32), 2),                          # host tensor
        lambda: bn254.fr_poly_quotients(z(3 * 32), z(2 * 32), 0),
        lambda: bn254.fr_poly_quotients(z(3 * 32), z(2 * 32), 1025),
        lambda: bn254.fr_poly_quotients(z(3 * 32), z(2 * 32), 2, stride=1),      # stride < B
        lambda: bn254.fr_poly_quotients(z(3 * 32), z(3 * 32), 2),                # points not a multiple of B
        lambda: bn254.fr_poly_quotients(z(2 * 32), z(2 * 32), 2),                # coeffs too short
        lambda: bn254.fr_poly_quotients(z(3 * 32), z(2 * 32), 2, out=z(3 * 32)),
        lambda: bn254.fr_poly_quotients(z(3 * 32), z(2 * 32), 2, ok=z(1)),
        lambda: bn254.fr_poly_quotients(z(3 * 32), t(2 * 32), 2),                # host / device mix
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()

    class Table:                                            # stands for an SRS table of B + 1 = 4 bases; never called
        nbase = 4
    for ids in (z(4 * 32), [[1, 2, 3], [4, 5]], [[1, 2, 2]], [[1, 2, 2 + fc.R]], z(0), t(5 * 32)):      # not a multiple of B; ragged; duplicated identity; empty
        for fn in (afp25.digests, afp25.opening_proofs):
            with pytest.raises(ValueError):
                fn(bn254, Table(), ids)
        with pytest.raises(ValueError):
            afp25.decrypt_batches(bn254, Table(), ids, z(64), z(3 * 3 * 128), z(3 * 384))


def test_c_entries_reject_invalid_arguments(lib):
    """GPBC_ERR_INVALID_ARG with a message, nothing written, before any device is touched; n = 0 / k = 0 is a no-op"""
    a, b, out = np.zeros(5 * 32, np.uint8), np.zeros(3 * 32, np.uint8), np.zeros(5 * 32, np.uint8)
    p = lambda x: VP(x.ctypes.data)
    for op in fc.BINARY:
        host, dev = getattr(lib, "gpbc_fr_%s_batch" % op), getattr(lib, "gpbc_fr_%s_batch_dev" % op)
        for rc in (host(p(a), p(b), SZ(3), SZ(5), p(out)), host(None, p(b), SZ(1), SZ(5), p(out)), host(p(a), None, SZ(5), SZ(5), p(out)),
                   host(p(a), p(b), SZ(5), SZ(5), None), dev(p(a), p(b), SZ(2), SZ(5), p(out), None), dev(None, p(b), SZ(1), SZ(5), p(out), None)):
            assert rc == -1 and lib.gpbc_last_error()
        assert host(None, None, SZ(0), SZ(0), None) == 0
    for op in fc.UNARY:
        host, dev = getattr(lib, "gpbc_fr_%s_batch" % op), getattr(lib, "gpbc_fr_%s_batch_dev" % op)
        assert host(None, SZ(4), p(out)) == -1 and host(p(a), SZ(4), None) == -1 and dev(None, SZ(4), p(out), None) == -1
        assert host(None, SZ(0), None) == 0 and dev(None, SZ(0), None, None) == 0
    big = np.zeros(4096, np.uint8)
    for B in (0, 1025):
        assert lib.gpbc_fr_poly_from_roots(p(big), SZ(B), SZ(1), p(big)) == -1 and b"B must be" in lib.gpbc_last_error()
        assert lib.gpbc_fr_poly_from_roots_dev(p(big), SZ(B), SZ(1), p(big), None) == -1
        assert lib.gpbc_fr_poly_quotients(p(big), p(big), SZ(B), SZ(1), SZ(2000), p(big), p(big)) == -1
        assert lib.gpbc_fr_poly_quotients_dev(p(big), p(big), SZ(B), SZ(1), SZ(2000), p(big), p(big), None) == -1
    assert lib.gpbc_fr_poly_quotients(p(big), p(big), SZ(4), SZ(1), SZ(3), p(big), p(big)) == -1 and b"stride" in lib.gpbc_last_error()
    assert lib.gpbc_fr_poly_quotients_dev(p(big), p(big), SZ(4), SZ(1), SZ(3), p(big), p(big), None) == -1
    for stride in ((1 << 24) + 1, 1 << 60, (1 << 64) - 1):                        # sizes that would overflow never reach an allocation
        assert lib.gpbc_fr_poly_quotients(p(big), p(big), SZ(4), SZ(1), SZ(stride), p(big), p(big)) == -1 and b"stride" in lib.gpbc_last_error()
        assert lib.gpbc_fr_poly_quotients_dev(p(big), p(big), SZ(4), SZ(1), SZ(stride), p(big), p(big), None) == -1
    assert lib.gpbc_fr_poly_from_roots(None, SZ(4), SZ(1), p(big)) == -1 and lib.gpbc_fr_poly_quotients(p(big), None, SZ(4), SZ(1), SZ(4), p(big), p(big)) == -1
    assert lib.gpbc_fr_poly_from_roots(None, SZ(4), SZ(0), None) == 0 and lib.gpbc_fr_poly_quotients(None, None, SZ(4), SZ(0), SZ(4), None, None) == 0
    assert not out.any() and not big.any()


def test_no_cpu_fallback_for_fr(lib):
    """without a GPU every new entry returns a negative status, writes nothing and leaves a message"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gopairingbasedcryptography_amd import bn254, EngineError
    a = fc.rows(fc.rand("nofb", 3))
    p = lambda x: VP(x.ctypes.data)
    for op in fc.BINARY + fc.UNARY:
        out = np.zeros_like(a)
        with pytest.raises(EngineError):
            getattr(bn254, "fr_" + op)(*((a, a) if op in fc.BINARY else (a,)), out=out)
        assert not out.any()
        host, dev = getattr(lib, "gpbc_fr_%s_batch" % op), getattr(lib, "gpbc_fr_%s_batch_dev" % op)
        rcs = (host(p(a), p(a), SZ(3), SZ(3), p(out)), dev(p(a), p(a), SZ(3), SZ(3), p(out), None)) if op in fc.BINARY else \
              (host(p(a), SZ(3), p(out)), dev(p(a), SZ(3), p(out), None))
        assert all(rc < 0 for rc in rcs) and not out.any() and lib.gpbc_last_error()
    co, q, ok = np.zeros((1, 4, 32), np.uint8), np.zeros((3, 4, 32), np.uint8), np.zeros(3, np.uint8)
    with pytest.raises(EngineError):
        bn254.fr_poly_from_roots([[1, 2, 3]], out=co)
    with pytest.raises(EngineError):
        bn254.fr_poly_quotients([6, 11, 6, 1], [1, 2, 3], 3, 4, out=q, ok=ok)
    assert lib.gpbc_fr_poly_from_roots(p(a), SZ(3), SZ(1), p(co)) < 0 and lib.gpbc_last_error()
    assert lib.gpbc_fr_poly_from_roots_dev(p(a), SZ(3), SZ(1), p(co), None) < 0
    assert lib.gpbc_fr_poly_quotients(p(q), p(a), SZ(3), SZ(1), SZ(4), p(q), p(ok)) < 0 and lib.gpbc_last_error()
    assert lib.gpbc_fr_poly_quotients_dev(p(q), p(a), SZ(3), SZ(1), SZ(4), p(q), p(ok), None) < 0
    assert not co.any() and not q.any() and not ok.any()
