"""The seven-product sparse line multiplication on the device (four products at c0 = 1): the throughput Miller kernels that use it
— k_miller_lines + k_miller_accumulate, k_miller_pipelined, k_miller_accumulate_fixed_q — and the chunk form beside them, against
the C oracle bit for bit.  The Miller VALUE is compared, not only the pairing: the doubled products leave a power of two on the
accumulator, which the constant of the last line must cancel exactly.  Sizes cross a 64-lane block (32 pairs).  Run with -m gpu."""
import numpy as np
import pytest

import bn254_py as o

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 33, 65)


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def scalars(tag, n):
    return np.frombuffer(b"".join(o.scalar_to_bytes(o.bench_scalar(tag, i)) for i in range(n)), dtype=np.uint8)


@pytest.fixture(scope="module")
def points(eng, oracle):
    """65 pairs: slot 3 has P at infinity, slot 40 has Q at infinity, slot 64 repeats slot 1; with the oracle's Miller values and pairings"""
    n = max(SIZES)
    g1, g2 = eng.generators()
    P = oracle.g1_scalar_mul(g1, scalars("sparse7-P", n), threads=8).reshape(n, 64).copy()
    Q = oracle.g2_scalar_mul(g2, scalars("sparse7-Q", n), threads=8).reshape(n, 128).copy()
    P[3] = 0
    Q[40] = 0
    P[64], Q[64] = P[1], Q[1]
    return P, Q, oracle.miller_loop(P, Q, threads=8), oracle.pair_batch(P, Q, threads=8)


@pytest.fixture
def throughput_kernels():
    """the latency form would take every call of this size (and the fixed-Q entry would skip its line table): switch it off"""
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    _lib.check(lib.gpbc_set_latency_path(0))
    yield lib
    lib.gpbc_set_pipelined_miller(1)
    lib.gpbc_set_latency_path(2048)


@pytest.mark.parametrize("pipelined", [0, 1], ids=["two_kernels", "pipelined"])
def test_miller_values_and_pairings(eng, points, throughput_kernels, pipelined):
    from gopairingbasedcryptography_amd import _lib
    P, Q, want_f, want_e = points
    _lib.check(throughput_kernels.gpbc_set_pipelined_miller(pipelined))
    one = np.frombuffer(o.gt_to_bytes(o.F12_ONE), dtype=np.uint8)
    for n in SIZES:
        f, e = eng.miller_loop(P[:n], Q[:n]), eng.pair_batch(P[:n], Q[:n])
        assert (f == want_f[:n]).all(), n
        assert (e == want_e[:n]).all(), n
    assert (f[3] == one).all() and (f[40] == one).all() and (e[3] == one).all() and (e[40] == one).all()
    assert (f[64] == f[1]).all() and (e[64] == e[1]).all()


def test_fixed_q_and_ragged_multi_pairings(eng, oracle, points, throughput_kernels):
    P, Q, _, _ = points
    k = 3
    for m in (1, 5, 9):                                    # three keys' worth of segments: k segments against one list of m G2 points
        Ps, Qs = P[4:4 + k * m].copy(), Q[4:4 + m].copy()
        off = np.arange(0, k * m + 1, m).astype(np.uint64)
        assert (eng.multi_pair_fixed_q(Ps, Qs) == oracle.multi_pair(Ps, np.tile(Qs, (k, 1)), off)).all(), m
    off = np.array([0, 1, 3, 12], dtype=np.uint64)         # ragged segments of 1, 2 and 9 pairs (P at infinity in the last one)
    assert (eng.multi_pair(P[:12], Q[:12], off) == oracle.multi_pair(P[:12], Q[:12], off)).all()
