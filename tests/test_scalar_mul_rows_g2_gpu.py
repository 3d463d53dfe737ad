"""The G2 row tables on the device (run with -m gpu; csrc/rows29_g2.hip.hpp, csrc/gpbc_rows_g2.hip): g2_scalar_mul with nbase bases for
nbase * m scalars through the host entry (numpy) and the _dev entry on a stream of its own, on the case table of tests/rows_cases.py
against the oracle's scalar multiplication on the expanded bases, bit for bit.  With T = ROWS_G2_TABLE_MIN the shapes are (3, T + 33) an
infinity base in the middle and waves that straddle two bases; (2, T - 1) and (2, T) both sides of the crossover; (65, T) build (b) across
workgroups; (65, 3) the tables forced at m = 3.  Every shape is also run with the tables forced and with the table-free kernel forced
(GPBC_ROWS_G2_TABLE_MIN, the measurement override): the same bytes.  Then one base more than a pass and than a group hold, against the
engine's own one-base-per-scalar call; and the names of the kernels a row call launched, which is what shows that the tables ran."""
import ctypes

import numpy as np
import pytest

import rows_cases as rcs
from gopairingbasedcryptography_amd import bn254 as constants

pytestmark = pytest.mark.gpu
KNOB = "GPBC_ROWS_G2_TABLE_MIN"
NEVER = constants.ROWS_G2_TABLE_MIN >= constants.ROWS_TABLE_MAX           # a crossover that keeps dispatch off the tables: the tests force them
T = 32 if NEVER else constants.ROWS_G2_TABLE_MIN
SHAPES = [(3, T + 33), (2, T - 1), (2, T), (65, T), (65, 3)]


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def as_built(monkeypatch):
    """the dispatch under test: the library's own crossover, or T through the override where the crossover would never take the tables"""
    if NEVER:
        monkeypatch.setenv(KNOB, str(T))
    else:
        monkeypatch.delenv(KNOB, raising=False)


def run(eng, b, k, form):
    if form == "host":
        out = eng.g2_scalar_mul(b, k)
        assert isinstance(out, np.ndarray)
        return out
    import torch
    db, dk = torch.from_numpy(np.ascontiguousarray(b)).cuda(), torch.from_numpy(np.ascontiguousarray(k)).cuda()
    torch.cuda.synchronize()
    if form == "dev":
        out = eng.g2_scalar_mul(db, dk)
        torch.cuda.synchronize()
    else:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            out = eng.g2_scalar_mul(db, dk)
        side.synchronize()
    assert out.is_cuda
    return out.cpu().numpy()


@pytest.mark.parametrize("form", ["host", "side-stream"])
@pytest.mark.parametrize("nbase,m", SHAPES)
def test_rows_against_the_oracle(eng, oracle, monkeypatch, nbase, m, form):
    as_built(monkeypatch)
    b, ks = rcs.bases(oracle, True, nbase), rcs.scalars(nbase, m)
    want = rcs.expected(oracle, True, nbase, m)
    out = run(eng, b, rcs.rows(ks), form).reshape(nbase * m, 128)
    bad = [i for i in range(nbase * m) if out[i].tobytes() != want[i].tobytes()]
    assert not bad, (bad[:8], [hex(ks[i]) for i in bad[:8]])
    if nbase >= 3:
        assert not out[m * rcs.INF_BASE:m * (rcs.INF_BASE + 1)].any()                   # the infinity base: a zero row


@pytest.mark.parametrize("nbase,m", SHAPES)
def test_both_routes_forced_give_the_same_bytes(eng, oracle, monkeypatch, nbase, m):
    b, k = rcs.bases(oracle, True, nbase), rcs.rows(rcs.scalars(nbase, m))
    monkeypatch.setenv(KNOB, "2")
    table = run(eng, b, k, "dev")
    monkeypatch.setenv(KNOB, "0")
    free = run(eng, b, k, "dev")
    assert table.tobytes() == free.tobytes() == rcs.expected(oracle, True, nbase, m).tobytes()


def test_one_base_more_than_a_pass_and_a_group_hold(eng, monkeypatch):
    """m = T, the shortest rows that take the tables: a pass is 2^18 outputs, the window bases are made for 2^16 bases at a time, so one
    base more than a group crosses every pass boundary of the group and the group boundary.  Against g2_scalar_mul with one base per
    scalar on the expanded bases, all on the device; a base at infinity first in the second pass and last overall."""
    import torch
    as_built(monkeypatch)
    pass_bases = constants.rows_g2_pass_bases(1 << 30, T)
    nbase = constants.ROWS_G2_GROUP_BASES + 1
    assert pass_bases == constants.ROWS_G2_PASS_OUTPUTS // T and nbase > pass_bases + 1 and T < constants.ROWS_TABLE_MAX
    rnd = np.random.default_rng(21)
    bases = eng.g2_scalar_mul_base(torch.from_numpy(rnd.integers(0, 256, (nbase, 32), dtype=np.uint8)).cuda()).reshape(nbase, 128)
    bases[5] = 0
    bases[pass_bases] = 0                                                         # the first base of the second pass
    bases[nbase - 1] = 0                                                          # the one base of the second group, the last overall
    bases[nbase - 2] = bases[0]
    k = torch.from_numpy(rnd.integers(0, 256, (nbase * T, 32), dtype=np.uint8)).cuda()
    got = eng.g2_scalar_mul(bases, k)
    want = eng.g2_scalar_mul(bases.repeat_interleave(T, dim=0).contiguous(), k)
    torch.cuda.synchronize()
    assert got.shape == (nbase * T, 128) and bool((got == want).all())
    rows = got.reshape(nbase, T, 128)
    assert not bool(rows[[5, pass_bases, nbase - 1]].any()) and bool(rows[nbase - 2].any()) and bool(rows[pass_bases - 1].any()) and bool(rows[pass_bases + 1].any())


def _profiled(eng, fn):
    """fn() and the names of the kernels it launched"""
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    _lib.check(lib.gpbc_profile_begin(eng._torch_stream()))
    out = fn()
    names, ms, cnt, nk = ctypes.create_string_buffer(32 * 16), (ctypes.c_double * 16)(), (ctypes.c_int * 16)(), ctypes.c_int(0)
    _lib.check(lib.gpbc_profile_end(names, ms, cnt, 16, ctypes.byref(nk)))
    return out, [names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode() for i in range(nk.value)]


def test_the_row_call_runs_the_table_kernels(eng, oracle, monkeypatch):
    """the route, by the names of the kernels launched: the G2 builds and evaluation and no table-free kernel from the crossover on; the
    other way round with the override at 0; G1's override does not move G2"""
    import torch
    m = max(T, 32)
    b = torch.from_numpy(rcs.bases(oracle, True, 3)).cuda()
    k = torch.from_numpy(rcs.rows(rcs.scalars(3, m))).cuda()
    as_built(monkeypatch)
    monkeypatch.setenv("GPBC_ROWS_TABLE_MIN", "0")
    table, names = _profiled(eng, lambda: eng.g2_scalar_mul(b, k))
    assert {"k_g2_rows_build_a", "k_g2_rows_build_b", "k_g2_rows_eval"} <= set(names) and "k_g2_rows_free" not in names, names
    monkeypatch.delenv("GPBC_ROWS_TABLE_MIN")
    monkeypatch.setenv(KNOB, "0")
    free, names = _profiled(eng, lambda: eng.g2_scalar_mul(b, k))
    assert "k_g2_rows_free" in names and not any(n.startswith("k_g2_rows_build") or n == "k_g2_rows_eval" for n in names), names
    torch.cuda.synchronize()
    assert bool(torch.equal(table, free))
