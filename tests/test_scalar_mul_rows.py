"""The lane functions of the row form of g1 / g2_scalar_mul (csrc/rows29.hip.hpp) as the kernels of csrc/gpbc_rows.hip launch them — build
(a) one lane per base, build (b) one lane per (base, window), the evaluation one lane per output, the table-free lane on base i / m —
compiled for the host with -DGPBC_BOUNDS (tools/rows_check.cpp) on the case table of tests/rows_cases.py, against the oracle's scalar
multiplication on the expanded bases, exactly.  Every product in that build asserts its int64 columns for ANY input of its interval
class, so a run that finishes is the limb-bound proof of the chains.  Then the argument rules of bn254._scalar_mul, which need no device."""
import os
import re

import numpy as np
import pytest

import rows_cases as rcs
import rows_harness
from conftest import ROOT
from rows_harness import rc  # noqa: F401  (the fixture)
from gopairingbasedcryptography_amd import bn254


def split_rows(splits):
    """(k1, k2, neg1, neg2) tuples -> the 12 uint32 per split of rc_eval_split / rc_glv_split"""
    words = lambda v: [(v >> (32 * i)) & 0xFFFFFFFF for i in range(5)]
    return np.array([words(k1) + words(k2) + [n1, n2] for k1, k2, n1, n2 in splits], dtype=np.uint32)


def run_table(rc, b, m, ks):
    table, inf = rows_harness.build_tables(rc, b)
    k = rcs.rows(ks)
    out = np.full((len(ks) + 1, 64), 0xA5, dtype=np.uint8)
    wide = rc.rc_eval(table.ctypes.data, inf.ctypes.data, len(b), m, k.ctypes.data, out.ctypes.data)
    assert wide == 0 and (out[len(ks)] == 0xA5).all()                  # no half beyond 128 bits, nothing past the end
    return out[:len(ks)], table, inf


def test_entries_and_geometry_are_what_the_modules_state(rc):
    src = open(os.path.join(ROOT, rows_harness.SRC)).read()
    assert sorted(set(re.findall(r"^(?:int|void|size_t) (rc_\w+)\(", src, flags=re.M))) == sorted(rows_harness.RC_SIGNATURES)
    geom = np.zeros(8, dtype=np.uint64)
    rc.rc_geometry(geom.ctypes.data)
    assert [int(v) for v in geom] == [32, 15, rows_harness.TABLE_BYTES, bn254.ROWS_TABLE_MIN, bn254.ROWS_PASS_OUTPUTS, bn254.ROWS_TABLE_CAP, rows_harness.WB_BYTES, bn254.ROWS_GROUP_BASES]
    assert rows_harness.TABLE_BYTES == bn254.ROWS_TABLE_BYTES == 32 * 15 * 128
    for nbase, m in ((1, 16), (3, 65), (16384, 16), (16385, 16), (1 << 20, 16), (1 << 20, 2), (1 << 20, 4096), (5, 1 << 19)):
        assert rc.rc_pass_bases(nbase, m) == bn254.rows_pass_bases(nbase, m) >= 1
        assert bn254.rows_pass_bases(nbase, m) * bn254.ROWS_TABLE_BYTES <= bn254.ROWS_TABLE_CAP
    assert bn254.rows_pass_bases(1 << 20, 16) == 16384                   # 2^18 outputs a pass, 960 MiB of tables


def test_corpus_covers_what_it_claims():
    assert set(rcs.PLANTED) <= set(rcs.scalars(3, 65)) and set(rcs.PLANTED) <= set(rcs.scalars(65, 3)) and set(rcs.SPECIAL) <= set(rcs.scalars(2, 16))
    assert len(rcs.SINGLES) == 64 and len(rcs.PLANTED) == 78 and len(set(rcs.PLANTED)) == 77          # window 0 of half one is the scalar 1 again
    assert pow(rcs.LAMBDA, 3, rcs.R) == 1 != rcs.LAMBDA


def test_split_restated_in_python_is_the_kernels(rc):
    ks = [k for nbase, m in rcs.SHAPES for k in rcs.scalars(nbase, m)]
    got, k = np.zeros((len(ks), 12), dtype=np.uint32), rcs.rows(ks)
    rc.rc_glv_split(k.ctypes.data, len(ks), got.ctypes.data)
    assert got.tolist() == split_rows([rcs.split(k) for k in ks]).tolist()
    assert all(rcs.split_scalar(rcs.split(k)) == k % rcs.R for k in ks)
    assert {(int(r[10]), int(r[11])) for r in got} == {(0, 0), (0, 1)}                   # what glv_split reaches; SPLITS covers the rest
    assert max(int(r[4]) | int(r[9]) for r in got) == 0                                   # the halves stay below 2^128
    for w in range(32):                                                                   # the planted half-one scalars ARE single nibbles
        k = rcs.SINGLES[2 * w]
        assert k < rcs.HALF_ONE_MAX and rcs.split(k) == (k, 0, 0, 0) and k >> (4 * w) in range(1, 16)


@pytest.mark.parametrize("nbase,m", rcs.SHAPES)
def test_row_tables_against_the_oracle(rc, oracle, nbase, m):
    b, ks = rcs.bases(oracle, False, nbase), rcs.scalars(nbase, m)
    got, table, inf = run_table(rc, b, m, ks)
    want = rcs.expected(oracle, False, nbase, m)
    bad = [i for i in range(nbase * m) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, (bad[:8], [hex(ks[i]) for i in bad[:8]])
    assert inf.tolist() == [1 if nbase >= 3 and j == rcs.INF_BASE else 0 for j in range(nbase)]
    per_base = table.view(np.uint8).reshape(nbase, -1)
    if nbase >= 3:
        assert (per_base[rcs.INF_BASE] == 0x5A).all() and not got[m:2 * m].any()            # no row written for it; its outputs are zero rows
    st = np.zeros(7)
    rc.rc_stats(st.ctypes.data)
    assert 0 < st[0] < 2.0**63 and st[1] < 2.0**31


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("nbase,m", rcs.SHAPES)
def test_table_free_rows_against_the_oracle(rc, oracle, g2, nbase, m):
    b, k = rcs.bases(oracle, g2, nbase), rcs.rows(rcs.scalars(nbase, m))
    width = 128 if g2 else 64
    out = np.full((nbase * m + 1, width), 0xA5, dtype=np.uint8)
    assert rc.rc_rows_free(int(g2), b.ctypes.data, nbase, m, k.ctypes.data, out.ctypes.data) == 0
    assert (out[nbase * m] == 0xA5).all()
    assert out[:nbase * m].tobytes() == rcs.expected(oracle, g2, nbase, m).tobytes()


def test_every_sign_window_and_digit_of_a_given_split(rc, oracle):
    """the walk on splits glv_split never returns: a single nibble per window of each half, every nibble 15, all four sign pairs"""
    b = rcs.bases(oracle, False, 2)
    table, inf = rows_harness.build_tables(rc, b)
    m = len(rcs.SPLITS)
    S = split_rows(rcs.SPLITS + rcs.SPLITS)
    out = np.zeros((2 * m, 64), dtype=np.uint8)
    assert rc.rc_eval_split(table.ctypes.data, inf.ctypes.data, 2, m, S.ctypes.data, out.ctypes.data) == 0
    want = rcs.expected_for(oracle, False, rcs.expand(b, m), [rcs.split_scalar(s) for s in rcs.SPLITS] * 2)
    bad = [i for i in range(2 * m) if out[i].tobytes() != want[i].tobytes()]
    assert not bad, [(i, rcs.SPLITS[i % m]) for i in bad[:8]]
    assert {(s[2], s[3]) for s in rcs.SPLITS} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(h, w) for h in (0, 1) for w in range(32)} == {(0 if s[0] else 1, (s[0] or s[1]).bit_length() - 1 >> 2) for s in rcs.SPLITS[:64]}


def test_the_whole_table_of_a_base(rc, oracle):
    """all 480 rows of a base, each read back through the walk as the one-digit split it serves: [d 16^w] P"""
    b = rcs.bases(oracle, False, 2)[1:]
    table, inf = rows_harness.build_tables(rc, b)
    singles = [(d << (4 * w), 0, 0, 0) for w in range(32) for d in range(1, 16)]
    out, S = np.zeros((len(singles), 64), dtype=np.uint8), split_rows(singles)
    assert rc.rc_eval_split(table.ctypes.data, inf.ctypes.data, 1, len(singles), S.ctypes.data, out.ctypes.data) == 0
    want = rcs.expected_for(oracle, False, rcs.expand(b, len(singles)), [s[0] for s in singles])
    assert out.tobytes() == want.tobytes()
    st = np.zeros(7)
    rc.rc_stats(st.ctypes.data)
    assert 0 < st[0] < 2.0**63 and st[1] < 2.0**31 and st[3] > 0


def test_harness_refuses_malformed_arguments(rc):
    table, wb, inf = rows_harness.table_memory(1)
    z = np.zeros(64, dtype=np.uint8)
    assert rc.rc_build_a(None, 1, wb.ctypes.data, inf.ctypes.data) == -1
    assert rc.rc_build_a(z.ctypes.data, 1, wb.ctypes.data + 16, inf.ctypes.data) == -1             # rows are 128-byte aligned
    assert rc.rc_build_b(None, table.ctypes.data, inf.ctypes.data, 1) == -1
    assert rc.rc_build_b(wb.ctypes.data, table.ctypes.data + 16, inf.ctypes.data, 1) == -1
    assert rc.rc_eval(table.ctypes.data, inf.ctypes.data, 1, 0, z.ctypes.data, z.ctypes.data) == -1
    assert rc.rc_eval_split(table.ctypes.data, None, 1, 1, z.ctypes.data, z.ctypes.data) == -1
    assert rc.rc_rows_free(0, z.ctypes.data, 1, 0, z.ctypes.data, z.ctypes.data) == -1


# ------------------------------------------------------------------------------------------------ bn254._scalar_mul, no device
@pytest.mark.parametrize("fn,width", [(bn254.g1_scalar_mul, 64), (bn254.g2_scalar_mul, 128)], ids=["g1", "g2"])
def test_base_counts_that_do_not_divide_still_raise(monkeypatch, fn, width):
    calls = []
    monkeypatch.setattr(bn254, "_call", lambda *a: calls.append(a))
    for nbase, n in ((2, 3), (4, 6), (3, 2), (7, 1), (5, 12)):
        with pytest.raises(ValueError, match="one base per row"):
            fn(np.zeros((nbase, width), dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8))
    with pytest.raises(ValueError):
        fn(np.zeros((0, width), dtype=np.uint8), np.zeros((4, 32), dtype=np.uint8))
    assert not calls                                                                     # refused before the engine is touched
    for nbase, n in ((1, 6), (6, 6), (2, 6), (3, 6), (3, 195)):
        out = fn(np.zeros((nbase, width), dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8))
        assert out.shape == (n, width) and calls[-1][0].endswith("_scalar_mul_batch") and calls[-1][3] == nbase and calls[-1][5] == n
