"""The one way into tools/libgpbc_rows_check.so, the row lane functions of csrc/rows29.hip.hpp compiled for the host with -DGPBC_BOUNDS
(tools/rows_check.cpp): built with the recipe of tests/bounds_harness.py, the C signature of every rc_* entry, and load(), which builds
the library when it is older than its sources and declares every entry.  Test modules take the `rc` fixture from here (not collected: no
test_ prefix)."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

from bounds_harness import CTYPES, RECIPE
from conftest import ROOT

SRC = os.path.join("tools", "rows_check.cpp")
SO = os.path.join("tools", "libgpbc_rows_check.so")
# the extern "C" entries of tools/rows_check.cpp in the notation of bounds_harness.HC_SIGNATURES (p pointer, z size_t, i int, v void)
RC_SIGNATURES = {
    "rc_geometry": "v:p", "rc_pass_bases": "z:zz", "rc_build_a": "i:pzpp", "rc_build_b": "i:pppz", "rc_eval": "i:ppzzpp", "rc_eval_split": "i:ppzzpp",
    "rc_glv_split": "v:pzp", "rc_rows_free": "i:ipzzpp", "rc_stats": "v:p",
}
TABLE_BYTES, WB_BYTES = 61440, 4096      # table rows / window bases per base; the harness reports them (rc_geometry) and test_scalar_mul_rows.py holds them together

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
    """tools/libgpbc_rows_check.so, rebuilt when it is older than rows_check.cpp or any csrc/*.hpp, loaded once per process, with every
    rc_* entry declared from RC_SIGNATURES"""
    global _lib
    if _lib is None:
        so = os.path.join(ROOT, SO)
        sources = [os.path.join(ROOT, SRC)] + glob.glob(os.path.join(ROOT, "gopairingbasedcryptography_amd", "csrc", "*.hpp"))
        if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in sources):
            build()
        lib = ctypes.CDLL(so)
        for name, sig in RC_SIGNATURES.items():
            ret, params = sig.split(":")
            fn = getattr(lib, name)
            fn.restype = CTYPES[ret]
            fn.argtypes = [CTYPES[k] for k in params]
        _lib = lib
    return _lib


@pytest.fixture(scope="module")
def rc():
    return load()


def aligned(nbytes):
    """nbytes of uint8, 128-byte aligned like the device's rows, filled with a pattern so that a row nobody wrote shows"""
    raw = np.full(nbytes + 128, 0x5A, dtype=np.uint8)
    off = (-raw.ctypes.data) % 128
    return raw[off:off + nbytes]


def table_memory(nbase):
    """(table as int32, window bases as int32, flags) for nbase bases"""
    return aligned(nbase * TABLE_BYTES).view(np.int32), aligned(nbase * WB_BYTES).view(np.int32), np.full(nbase, 7, dtype=np.uint8)


def build_tables(rc, bases):
    """build (a) then build (b) over [nbase, 64] bases -> (table, inf)"""
    b = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1, 64)
    table, wb, inf = table_memory(len(b))
    assert rc.rc_build_a(b.ctypes.data, len(b), wb.ctypes.data, inf.ctypes.data) == 0
    assert (table.view(np.uint8) == 0x5A).all()                          # (a) writes window bases and flags only
    assert rc.rc_build_b(wb.ctypes.data, table.ctypes.data, inf.ctypes.data, len(b)) == 0
    return table, inf
