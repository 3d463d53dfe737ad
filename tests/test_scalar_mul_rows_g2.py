"""The lane functions of the G2 row tables (csrc/rows29_g2.hip.hpp) as the kernels of csrc/gpbc_rows_g2.hip launch them — build (a) one
lane per base, build (b) one lane per (base, window), the evaluation one lane per output with psi applied to the accumulator between the
GLS quarters — compiled for the host with -DGPBC_BOUNDS (tools/rows_g2_check.cpp), against the oracle's G2 scalar multiplication on the
expanded bases, exactly.  Every product in that build asserts its int64 columns for ANY input of its interval class, so a run that
finishes is the limb-bound proof of both builds and of the walk, the psi step included.  `wide` (a quarter beyond the 17 windows) is
never set on any case."""
import os
import re

import numpy as np
import pytest

import rows_cases as rcs
import rows_g2_cases as gcs
import rows_g2_harness
from conftest import ROOT
from rows_g2_harness import rg  # noqa: F401  (the fixture)
from gopairingbasedcryptography_amd import bn254

NBASE = 3                                                               # the generator, the point at infinity, a random point


def bases(oracle):
    return rcs.bases(oracle, True, NBASE)


@pytest.fixture(scope="module")
def tables(rg, oracle):
    return rows_g2_harness.build_tables(rg, bases(oracle))


def check_stats(rg):
    st = np.zeros(7)
    rg.rg_stats(st.ctypes.data)
    assert 0 < st[0] < 2.0**63 and st[1] < 2.0**31 and st[3] > 0


def eval_scalars(rg, tables, m, ks):
    table, inf = tables
    k = rcs.rows(ks)
    out = np.full((len(ks) + 1, 128), 0xA5, dtype=np.uint8)
    wide = rg.rg_eval(table.ctypes.data, inf.ctypes.data, len(ks) // m, m, k.ctypes.data, out.ctypes.data)
    assert wide == 0 and (out[len(ks)] == 0xA5).all()                  # no quarter beyond 68 bits, nothing past the end
    return out[:len(ks)]


def eval_splits(rg, tables, splits):
    """every split on every base: [NBASE * len(splits), 128]"""
    table, inf = tables
    S = gcs.split_rows(list(splits) * NBASE)
    out = np.zeros((len(S), 128), dtype=np.uint8)
    assert rg.rg_eval_split(table.ctypes.data, inf.ctypes.data, NBASE, len(splits), S.ctypes.data, out.ctypes.data) == 0
    return out


def test_entries_and_geometry_are_what_the_modules_state(rg):
    src = open(os.path.join(ROOT, rows_g2_harness.SRC)).read()
    assert sorted(set(re.findall(r"^(?:int|void|size_t) (rg_\w+)\(", src, flags=re.M))) == sorted(rows_g2_harness.RG_SIGNATURES)
    geom = np.zeros(8, dtype=np.uint64)
    rg.rg_geometry(geom.ctypes.data)
    assert [int(v) for v in geom] == [17, 15, rows_g2_harness.TABLE_BYTES, bn254.ROWS_G2_TABLE_MIN, bn254.ROWS_G2_PASS_OUTPUTS, bn254.ROWS_G2_TABLE_CAP,
                                      rows_g2_harness.WB_BYTES, bn254.ROWS_G2_GROUP_BASES]
    assert rows_g2_harness.TABLE_BYTES == bn254.ROWS_G2_TABLE_BYTES == 17 * 15 * 256 and rows_g2_harness.WB_BYTES == 17 * 256
    for nbase, m in ((1, 16), (3, 65), (8192, 32), (8193, 32), (16448, 8), (16449, 8), (1 << 20, 2), (1 << 20, 4096), (5, 1 << 19)):
        assert rg.rg_pass_bases(nbase, m) == bn254.rows_g2_pass_bases(nbase, m) >= 1
        assert bn254.rows_g2_pass_bases(nbase, m) * bn254.ROWS_G2_TABLE_BYTES <= bn254.ROWS_G2_TABLE_CAP
    assert bn254.rows_g2_pass_bases(1 << 20, 32) == 8192                 # 2^18 outputs a pass, 510 MiB of tables
    assert bn254.rows_g2_pass_bases(1 << 20, 8) == (1 << 30) // 65280 == 16448           # the cap on the tables' bytes
    assert bn254.ROWS_TABLE_MIN == 32 and bn254.ROWS_TABLE_BYTES == 61440              # G1 keeps its own


def test_build_writes_every_row_of_every_base(rg, oracle, tables):
    """all 255 rows of each base, read back through the walk as the one-digit split each serves: [d 16^w] P; the base at infinity gets a
    flag and no row"""
    table, inf = tables
    assert inf.tolist() == [0, 1, 0]
    per_base = table.view(np.uint8).reshape(NBASE, -1)
    assert (per_base[rcs.INF_BASE] == 0x5A).all() and not (per_base[0].reshape(255, 256)[:, :160] == 0x5A).all(axis=1).any()
    singles = [(d << (4 * w), 0, 0, 0, 0, 0, 0, 0) for w in range(17) for d in range(1, 16)]
    out = eval_splits(rg, tables, singles)
    want = rcs.expected_for(oracle, True, rcs.expand(bases(oracle), len(singles)), [s[0] for s in singles] * NBASE)
    assert out.tobytes() == want.tobytes()
    check_stats(rg)


def test_every_sign_window_and_digit_of_a_given_split(rg, oracle, tables):
    out = eval_splits(rg, tables, gcs.SPLITS)
    m = len(gcs.SPLITS)
    want = rcs.expected_for(oracle, True, rcs.expand(bases(oracle), m), [gcs.split_scalar(s) for s in gcs.SPLITS] * NBASE)
    bad = [i for i in range(NBASE * m) if out[i].tobytes() != want[i].tobytes()]
    assert not bad, [(i, gcs.SPLITS[i % m]) for i in bad[:8]]
    # what the list claims to hold
    assert {(i, (s[i].bit_length() - 1) >> 2, s[4 + i]) for s in gcs.SINGLES for i in range(4) if s[i]} == {(i, w, n) for i in range(4) for w in range(17) for n in (0, 1)}
    assert {s[4:] for s in gcs.FULL} == {tuple((v >> i) & 1 for i in range(4)) for v in range(16)} and all(s[:4] == ((1 << 66) - 1,) * 4 for s in gcs.FULL)
    first = gcs.SPLITS.index(gcs.CANCEL[0])
    assert not out[first].any() and not out[first + 1].any() and out[first + 2].any() and out[first + 3].any()         # P - P, and the restart after it
    assert not out[m:2 * m].any()                                        # the base at infinity
    check_stats(rg)


def test_scalars_through_gls_split(rg, oracle, tables):
    per_row = rcs.SPECIAL + gcs.SCALARS_MU + gcs.random_scalars(40)
    m = len(per_row)
    ks = per_row * NBASE
    out = eval_scalars(rg, tables, m, ks)
    want = rcs.expected_for(oracle, True, rcs.expand(bases(oracle), m), ks)
    bad = [i for i in range(len(ks)) if out[i].tobytes() != want[i].tobytes()]
    assert not bad, (bad[:8], [hex(ks[i]) for i in bad[:8]])
    # the split is the decomposition the cases module states, and its quarters stay below 2^66
    got, k = np.zeros((m, 16), dtype=np.uint32), rcs.rows(per_row)
    rg.rg_gls_split(k.ctypes.data, m, got.ctypes.data)
    splits = [gcs.rows_split(r) for r in got]
    assert all(gcs.split_scalar(s) == v % rcs.R for s, v in zip(splits, per_row))
    assert max(max(s[:4]) for s in splits) < 1 << 66
    check_stats(rg)


@pytest.mark.parametrize("nbase,m", rcs.SHAPES)
def test_row_tables_against_the_oracle(rg, oracle, nbase, m):
    """the shapes and planted scalars of the G1 harness test, and the bytes the table-free route is held to"""
    b, ks = rcs.bases(oracle, True, nbase), rcs.scalars(nbase, m)
    t = rows_g2_harness.build_tables(rg, b)
    out = eval_scalars(rg, t, m, ks)
    want = rcs.expected(oracle, True, nbase, m)
    bad = [i for i in range(nbase * m) if out[i].tobytes() != want[i].tobytes()]
    assert not bad, (bad[:8], [hex(ks[i]) for i in bad[:8]])
    assert t[1].tolist() == [1 if nbase >= 3 and j == rcs.INF_BASE else 0 for j in range(nbase)]
    check_stats(rg)


def test_harness_refuses_malformed_arguments(rg):
    table, wb, inf = rows_g2_harness.table_memory(1)
    z = np.zeros(128, dtype=np.uint8)
    assert rg.rg_build_a(None, 1, wb.ctypes.data, inf.ctypes.data) == -1
    assert rg.rg_build_a(z.ctypes.data, 1, wb.ctypes.data + 16, inf.ctypes.data) == -1             # rows are 256-byte aligned
    assert rg.rg_build_b(None, table.ctypes.data, inf.ctypes.data, 1) == -1
    assert rg.rg_build_b(wb.ctypes.data, table.ctypes.data + 16, inf.ctypes.data, 1) == -1
    assert rg.rg_eval(table.ctypes.data, inf.ctypes.data, 1, 0, z.ctypes.data, z.ctypes.data) == -1
    assert rg.rg_eval_split(table.ctypes.data, None, 1, 1, z.ctypes.data, z.ctypes.data) == -1
