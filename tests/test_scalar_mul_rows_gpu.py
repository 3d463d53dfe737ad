"""The row form of g1 / g2_scalar_mul on the device (run with -m gpu): nbase bases for nbase * m scalars through the host entry (numpy) and
the _dev entry (CUDA tensors on a stream of their own), G1 and G2, on the case table of tests/rows_cases.py against the oracle's scalar
multiplication on the expanded bases, bit for bit.  Shapes: (3, 65) a wave straddles bases; (65, 3) more than one wave of bases, the
table-free route; (2, ROWS_TABLE_MIN - 1) and (2, ROWS_TABLE_MIN) both sides of the crossover; (65, ROWS_TABLE_MIN) build (b) beyond
one wave.  Then one base more than a pass of the row tables holds, against the engine's own one-base-per-scalar call; the refusals of
the C entries; and both routes forced through the measurement override."""
import numpy as np
import pytest

import rows_cases as rcs
from gopairingbasedcryptography_amd import bn254 as constants

pytestmark = pytest.mark.gpu
TMIN = constants.ROWS_TABLE_MIN
SHAPES = [(3, 65), (65, 3), (2, TMIN - 1), (2, TMIN), (65, TMIN)]


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def run(eng, g2, b, k, form):
    fn = eng.g2_scalar_mul if g2 else eng.g1_scalar_mul
    if form == "host":
        out = fn(b, k)
        assert isinstance(out, np.ndarray)
        return out
    import torch
    db, dk = torch.from_numpy(np.ascontiguousarray(b)).cuda(), torch.from_numpy(np.ascontiguousarray(k)).cuda()
    torch.cuda.synchronize()
    if form == "dev":
        out = fn(db, dk)
        torch.cuda.synchronize()
    else:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            out = fn(db, dk)
        side.synchronize()
    assert out.is_cuda
    return out.cpu().numpy()


@pytest.mark.parametrize("form", ["host", "dev", "side-stream"])
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("nbase,m", SHAPES)
def test_rows_against_the_oracle(eng, oracle, nbase, m, g2, form):
    b, ks = rcs.bases(oracle, g2, nbase), rcs.scalars(nbase, m)
    want = rcs.expected(oracle, g2, nbase, m)
    out = run(eng, g2, b, rcs.rows(ks), form).reshape(nbase * m, -1)
    bad = [i for i in range(nbase * m) if out[i].tobytes() != want[i].tobytes()]
    assert not bad, (bad[:8], [hex(ks[i]) for i in bad[:8]])
    if nbase >= 3:
        assert not out[m * rcs.INF_BASE:m * (rcs.INF_BASE + 1)].any()                   # the infinity base: a zero row


def test_the_row_call_is_the_call_on_the_repeated_bases(eng, oracle):
    """the same canonical bytes as nbase == n on the bases repeated m times, on both sides of the crossover and in both groups"""
    for g2 in (False, True):
        for nbase, m in ((65, TMIN), (65, 3)):
            b, k = rcs.bases(oracle, g2, nbase), rcs.rows(rcs.scalars(nbase, m))
            fn = eng.g2_scalar_mul if g2 else eng.g1_scalar_mul
            assert np.asarray(fn(b, k)).tobytes() == np.asarray(fn(rcs.expand(b, m), k)).tobytes()


def test_one_base_more_than_a_pass_and_a_group_hold(eng):
    """The shortest rows that take the tables (m = ROWS_TABLE_MIN; 16 when the tables started there): a pass is 2^18 outputs, the window
    bases are made for 2^16 bases at a time, so one base more than that crosses every pass boundary of a group and the group boundary.
    Against g1_scalar_mul with one base per scalar on the expanded bases, all on the device; a base at infinity in the first and the
    last pass."""
    import torch
    m = max(16, constants.ROWS_TABLE_MIN)
    pass_bases = constants.rows_pass_bases(1 << 30, m)
    nbase = constants.ROWS_GROUP_BASES + 1
    assert pass_bases == constants.ROWS_PASS_OUTPUTS // m and nbase > pass_bases + 1 and constants.ROWS_TABLE_MIN <= m < constants.ROWS_TABLE_MAX
    rnd = np.random.default_rng(20)
    bases = eng.g1_scalar_mul_base(torch.from_numpy(rnd.integers(0, 256, (nbase, 32), dtype=np.uint8)).cuda()).reshape(nbase, 64)
    bases[5] = 0
    bases[pass_bases] = 0                                                         # the first base of the second pass
    bases[nbase - 1] = 0                                                          # the one base of the second group
    bases[nbase - 2] = bases[0]
    k = torch.from_numpy(rnd.integers(0, 256, (nbase * m, 32), dtype=np.uint8)).cuda()
    got = eng.g1_scalar_mul(bases, k)
    want = eng.g1_scalar_mul(bases.repeat_interleave(m, dim=0).contiguous(), k)
    torch.cuda.synchronize()
    assert got.shape == (nbase * m, 64) and bool((got == want).all())
    assert not bool(got.reshape(nbase, m, 64)[[5, pass_bases, nbase - 1]].any()) and bool(got.reshape(nbase, m, 64)[nbase - 2].any())


def test_both_routes_forced_give_the_same_bytes(eng, oracle, monkeypatch):
    """GPBC_ROWS_TABLE_MIN (the measurement override of csrc/gpbc_rows.hip): the tables at m = 3, the table-free kernel at m = ROWS_TABLE_MIN"""
    for value, (nbase, m) in (("2", (65, 3)), ("0", (65, TMIN))):
        monkeypatch.setenv("GPBC_ROWS_TABLE_MIN", value)
        out = run(eng, False, rcs.bases(oracle, False, nbase), rcs.rows(rcs.scalars(nbase, m)), "dev")
        assert out.tobytes() == rcs.expected(oracle, False, nbase, m).tobytes(), (value, nbase, m)


def test_other_base_counts_are_refused_with_nothing_written(eng):
    import torch
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    for g2 in (False, True):
        width, name = (128, "gpbc_g2_scalar_mul_batch") if g2 else (64, "gpbc_g1_scalar_mul_batch")
        for nbase, n in ((2, 3), (4, 6), (7, 6), (0, 6)):
            b, k, out = np.zeros((8, width), np.uint8), np.ones((n, 32), np.uint8), np.full((n, width), 0xA5, np.uint8)
            assert getattr(lib, name)(b.ctypes.data, nbase, k.ctypes.data, n, out.ctypes.data) == -1                        # GPBC_ERR_INVALID_ARG
            assert (out == 0xA5).all() and b"divisor of n" in lib.gpbc_last_error()
            db, dk, do = torch.from_numpy(b).cuda(), torch.from_numpy(k).cuda(), torch.from_numpy(out).cuda()
            assert getattr(lib, name + "_dev")(db.data_ptr(), nbase, dk.data_ptr(), n, do.data_ptr(), None) == -1
            torch.cuda.synchronize()
            assert bool((do == 0xA5).all())
        with pytest.raises(ValueError):
            (eng.g2_scalar_mul if g2 else eng.g1_scalar_mul)(np.zeros((2, width), np.uint8), np.zeros((3, 32), np.uint8))
