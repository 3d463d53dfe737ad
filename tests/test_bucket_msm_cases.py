"""CPU part of the structured bucket-MSM cases (tests/msm_bucket_cases.py; the device part is tests/test_bucket_msm_structured_gpu.py):
  * every case, at the smallest shape of each plan (c = 12 just above MSM_MIN_TERMS, c = 16 just above 2^17), keeps its longest bucket
    at or below HALF of what msm_run accepts — k_msm_keys restated in numpy — so that the device call stays on the bucket path;
  * the log model confirms that every case triggers the events it is named after (and reproduces sum a_i k_i, which checks the model);
  * every skeleton rebuilt for c = 5 and c = 8 with a few dozen filler pairs runs through msm_host under the bounds harness (the
    per-lane pieces of csrc/msm29.hip.hpp, overflow-free on these inputs) and equals the oracle's sum of scalar multiplications and
    [sum a_i k_i]G.  msm_host has no sub-buckets: these cases carry plain top digits."""
import ctypes

import numpy as np
import pytest

import bn254_py as o
import msm_bucket_cases as mc
from bounds_harness import hc  # noqa: F401  (the fixture)

DEVICE = mc.case_ids(mc.SHAPES, "device")
REDUCED = mc.case_ids(mc.REDUCED, "host")


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_restated_keys_and_negation():
    """digits() against Python's shifts, the sub-bucket bits of the partial top window, and p - y on stored residues"""
    rng = np.random.default_rng(7)
    K = rng.integers(0, 256, size=(600, 32), dtype=np.uint8)
    K[0] = 0; K[1] = 255
    ks = [int.from_bytes(K[i].tobytes(), "little") for i in range(600)]
    for c in (5, 8, 12, 16):
        D = mc.digits(K, c)
        assert D.shape == (600, mc.n_windows(c))
        assert all(int(D[i, w]) == (ks[i] >> (c * w)) & ((1 << c) - 1) for i in range(600) for w in range(D.shape[1])), c
    inf = np.zeros(600, dtype=bool); inf[5] = True
    D12, plain = mc.keys(K, inf, 12), mc.digits(K, 12)
    assert (D12[:, :-1] == np.where(inf[:, None], 0, plain[:, :-1])).all() and not D12[5].any() and not D12[0].any()
    live = (plain[:, -1] != 0) & ~inf
    assert (D12[live, -1] == (np.arange(600)[live] % 256) * 16 + plain[live, -1]).all() and not D12[~live, -1].any()
    assert (mc.keys(K, inf, 16)[~inf] == mc.digits(K, 16)[~inf]).all()             # c = 16 has no partial window
    assert mc.bucket_cap(16390, 12) == 288 and mc.bucket_cap(131078, 16) == 272 and mc.window_bits(131071) == 12 and mc.window_bits(131072) == 16
    ys = [0, 1, o.P - 1, (1 << 64), (1 << 128) - 1, o.P - (1 << 192)] + [int.from_bytes(rng.bytes(32), "little") % o.P for _ in range(50)]
    rows = np.frombuffer(b"".join(y.to_bytes(32, "little") for y in ys), dtype=np.uint8).reshape(-1, 64)       # two values per row, as G2's y
    assert mc.negate_rows(rows).tobytes() == b"".join(((o.P - y) % o.P).to_bytes(32, "little") for y in ys)


@pytest.mark.parametrize("name,c,n", DEVICE)
def test_longest_bucket_at_most_half_the_cap(name, c, n):
    case = mc.build(name, c, n)
    assert case.n == n >= mc.MSM_MIN_TERMS and mc.window_bits(n) == c
    longest = mc.longest_bucket(case.keys(), c)
    print("%s c=%d n=%d: longest bucket %d, cap %d" % (name, c, n, longest, mc.bucket_cap(n, c)))
    assert 2 * longest <= mc.bucket_cap(n, c), (name, c, n, longest)


@pytest.mark.parametrize("name,c,n", DEVICE)
def test_log_model_certifies_the_case(name, c, n):
    case = mc.build(name, c, n)
    m = mc.Model(case)
    print("%s c=%d n=%d: %s" % (name, c, n, m.counts()))
    assert mc.certify(case, m) == [], (name, c, n, m.counts())


@pytest.mark.parametrize("name,c,n", REDUCED)
def test_reduced_case_through_msm_host_under_bounds(hc, oracle, name, c, n):
    case = mc.build(name, c, n, "host")
    m = mc.Model(case)
    assert mc.certify(case, m) == [], (name, c, n, m.counts())
    g1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
    g2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
    K = case.scalars
    for is_g2, gen, mul, summ, w in ((0, g1, oracle.g1_scalar_mul, oracle.g1_sum, 64), (1, g2, oracle.g2_scalar_mul, oracle.g2_sum, 128)):
        B = mc.base_rows(case, w, lambda rows: mul(gen, rows.reshape(-1)))
        want = np.asarray(summ(mul(B.reshape(-1), K.reshape(-1)))).reshape(-1)
        assert (want == np.asarray(mul(gen, mc.log_rows([case.expect_log]).reshape(-1))).reshape(-1)).all(), (name, c, w, "oracle sum against the known log")
        out = np.full(w, 0x5A, dtype=np.uint8)
        hc.hc_msm(ctypes.c_int(is_g2), vp(B), vp(K), ctypes.c_size_t(n), ctypes.c_int(c), vp(out))
        assert (out == want).all(), (name, c, w)
