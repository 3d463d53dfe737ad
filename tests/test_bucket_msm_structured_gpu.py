"""The exceptional group-law cases of the bucket (Pippenger) MSM ON the bucket path (run with -m gpu): every case of
tests/msm_bucket_cases.py — one base, P and -P, cancelling pairs in both layouts, pairs plus a lone term, a sum that closes to zero, the
group reduction with total = -running and with an infinite running sum under the 2^c - 9 multiplier (and inside the partial top
window), equal and opposite group rows in the tree, Horner steps that must double or give infinity mid-chain, top-window digits only,
bases at infinity — in G1 and G2, at the smallest shape of each window size, through gpbc_g1/g2_scalar_mul_sum_dev with CUDA tensors
and, for c = 12, through the host entry.
  * The expected bytes are [sum a_i k_i mod r]G from the oracle: the bases are [a_i]G with known a_i (ScalarMultiplicationBase, a slice
    checked against the oracle; negatives are p - y in numpy).  Nothing expected comes from the engine's sums.
  * gpbc_msm_stats must advance by exactly one bucket run and no fallback per call: the path is asserted, not assumed.
  * tests/test_bucket_msm_cases.py certifies on the CPU that each case triggers the events it is named after and stays under half the
    skew cap."""
import ctypes

import numpy as np
import pytest

import msm_bucket_cases as mc

pytestmark = pytest.mark.gpu

CASES = [(name, c, n, g2) for name, c, n in mc.case_ids(mc.SHAPES, "device") for g2 in (False, True)]


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def paths():
    """(bucket runs, skew fallbacks) so far"""
    from gopairingbasedcryptography_amd import _lib
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(_lib.load().gpbc_msm_stats(ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


@pytest.fixture(scope="module")
def group(eng, oracle):
    """g2 -> (width, [s]G by the engine's tables, [s]G by the oracle, the points of msm_bucket_cases.pool()); the pool's points are
    computed once per group, and 300 of their rows — half of them negated by negate_rows — are held against the oracle"""
    made = {}
    def get(g2):
        if g2 not in made:
            w = 128 if g2 else 64
            gen = eng.generators()[1 if g2 else 0]
            omul = oracle.g2_scalar_mul if g2 else oracle.g1_scalar_mul
            base = lambda rows: np.asarray((eng.g2_scalar_mul_base if g2 else eng.g1_scalar_mul_base)(np.ascontiguousarray(rows).reshape(-1))).reshape(-1, w)
            exact = lambda rows: np.asarray(omul(gen, np.ascontiguousarray(rows).reshape(-1), threads=16)).reshape(-1, w)
            logs = mc.pool()
            pts = base(mc.log_rows(logs))
            pick = list(range(0, mc.POOL_SIZE, mc.POOL_SIZE // 300))[:300]
            got = pts[pick].copy()
            got[150:, w // 2:] = mc.negate_rows(got[150:, w // 2:])
            assert (got == exact(mc.log_rows([logs[j] if t < 150 else mc.R - logs[j] for t, j in enumerate(pick)]))).all(), ("pool points", g2)
            made[g2] = (w, base, exact, pts)
        return made[g2]
    return get


@pytest.mark.parametrize("name,c,n,g2", CASES)
def test_structured_case_on_the_bucket_path(eng, group, name, c, n, g2):
    import torch
    w, base, exact, pool_points = group(g2)
    case = mc.build(name, c, n)
    checked = []
    def own(rows):                                                        # the case's own few points: every one against the oracle
        pts = base(rows)
        if len(rows) <= 16:
            assert (pts == exact(rows)).all(), (name, "skeleton points")
            checked.append(len(rows))
        return pts
    B = mc.base_rows(case, w, own, pool_points)
    assert checked or not (case.src < 0).any()
    want = exact(mc.log_rows([case.expect_log]))[0]
    if name.startswith("pairs_only") or name == "sum_zero_closing":
        assert not want.any() and want.size == w                          # 64 / 128 zero bytes
    msm = eng.g2_scalar_mul_sum if g2 else eng.g1_scalar_mul_sum
    dB, dK = torch.from_numpy(B).cuda(), torch.from_numpy(case.scalars).cuda()
    before = paths()
    got = msm(dB.reshape(-1), dK.reshape(-1)).cpu().numpy().reshape(-1)
    after = paths()
    assert after == (before[0] + 1, before[1]), ("the case must run the bucket method, not the per-term fallback", name, c, n, g2, before, after)
    assert (got == want).all(), (name, c, n, g2, "device entry")
    if c == 12:
        before = paths()
        got_h = np.asarray(msm(B.reshape(-1), case.scalars.reshape(-1))).reshape(-1)
        if eng.num_devices() == 1:                                        # the host entry shards over the bound devices
            assert paths() == (before[0] + 1, before[1]), (name, c, n, g2, "host entry path")
        assert (got_h == want).all(), (name, c, n, g2, "host entry")
