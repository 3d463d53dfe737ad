"""The one way into tools/libgpbc_rows_g2_check.so, the G2 row lane functions of csrc/rows29_g2.hip.hpp compiled for the host with
-DGPBC_BOUNDS (tools/rows_g2_check.cpp): built with the recipe of tests/bounds_harness.py, the C signature of every rg_* entry, and
load(), which builds the library when it is older than its sources and declares every entry.  Test modules take the `rg` fixture from
here (not collected: no test_ prefix)."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

from bounds_harness import CTYPES, RECIPE
from conftest import ROOT

SRC = os.path.join("tools", "rows_g2_check.cpp")
SO = os.path.join("tools", "libgpbc_rows_g2_check.so")
# the extern "C" entries of tools/rows_g2_check.cpp in the notation of bounds_harness.HC_SIGNATURES (p pointer, z size_t, i int, v void)
RG_SIGNATURES = {
    "rg_geometry": "v:p", "rg_pass_bases": "z:zz", "rg_build_a": "i:pzpp", "rg_build_b": "i:pppz", "rg_eval": "i:ppzzpp", "rg_eval_split": "i:ppzzpp",
    "rg_gls_split": "v:pzp", "rg_stats": "v:p",
}
WINDOWS, DIGITS = 17, 15
TABLE_BYTES, WB_BYTES = 65280, 4352      # table rows / window bases per base; the harness reports them (rg_geometry) and test_scalar_mul_rows_g2.py holds them together

_lib = None


def build():
    """compile to a name of its own, then move into place, as bounds_harness.build does"""
    so = os.path.join(ROOT, SO)
    tmp = "%s.%d.tmp" % (so, os.getpid())
    try:
        subprocess.check_call(RECIPE + ["-o", tmp, os.path.join(ROOT, SRC)])
        os.replace(tmp, so)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def load():
    """tools/libgpbc_rows_g2_check.so, rebuilt when it is older than rows_g2_check.cpp or any csrc/*.hpp, loaded once per process, with
    every rg_* entry declared from RG_SIGNATURES"""
    global _lib
    if _lib is None:
        so = os.path.join(ROOT, SO)
        sources = [os.path.join(ROOT, SRC)] + glob.glob(os.path.join(ROOT, "gopairingbasedcryptography_amd", "csrc", "*.hpp"))
        if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in sources):
            build()
        lib = ctypes.CDLL(so)
        for name, sig in RG_SIGNATURES.items():
            ret, params = sig.split(":")
            fn = getattr(lib, name)
            fn.restype = CTYPES[ret]
            fn.argtypes = [CTYPES[k] for k in params]
        _lib = lib
    return _lib


@pytest.fixture(scope="module")
def rg():
    return load()


def aligned(nbytes):
    """nbytes of uint8, 256-byte aligned like the device's rows, filled with a pattern so that a row nobody wrote shows"""
    raw = np.full(nbytes + 256, 0x5A, dtype=np.uint8)
    off = (-raw.ctypes.data) % 256
    return raw[off:off + nbytes]


def table_memory(nbase):
    """(table as int32, window bases as int32, flags) for nbase bases"""
    return aligned(nbase * TABLE_BYTES).view(np.int32), aligned(nbase * WB_BYTES).view(np.int32), np.full(nbase, 7, dtype=np.uint8)


def build_tables(rg, bases):
    """build (a) then build (b) over [nbase, 128] bases -> (table, inf)"""
    b = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1, 128)
    table, wb, inf = table_memory(len(b))
    assert rg.rg_build_a(b.ctypes.data, len(b), wb.ctypes.data, inf.ctypes.data) == 0
    assert (table.view(np.uint8) == 0x5A).all()                          # (a) writes window bases and flags only
    assert set(inf.tolist()) <= {0, 1}
    assert rg.rg_build_b(wb.ctypes.data, table.ctypes.data, inf.ctypes.data, len(b)) == 0
    return table, inf
