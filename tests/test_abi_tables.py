"""The whole C ABI surface on the CPU: every public header against its table in _lib.HEADERS and against what load() declared, the
tables against each other and against the exports of the built library, and the build lists of _build against the files they name.
What is specific to one header (its exact symbol list, its citations, where its kernels live) stays in that feature's own test module."""
import glob
import os
import re
import subprocess

import pytest

from conftest import ROOT
import abi_headers
from gopairingbasedcryptography_amd import _build, _lib

MAIN = "gpbc_bn254.h"
# header -> (its version entry, the value that entry returns)
VERSIONS = {
    "gpbc_bn254.h": ("gpbc_abi_version", 8), "gpbc_bn254_ext.h": ("gpbc_ext_version", 2), "gpbc_bn254_subset.h": ("gpbc_subset_version", 1),
    "gpbc_bn254_hash.h": ("gpbc_hash_version", 1), "gpbc_bn254_share.h": ("gpbc_share_version", 1), "gpbc_bn254_indexed.h": ("gpbc_indexed_version", 1),
    "gpbc_bn254_recon.h": ("gpbc_recon_version", 1), "gpbc_bn254_select.h": ("gpbc_select_version", 1), "gpbc_bn254_formula.h": ("gpbc_formula_version", 1),
    "gpbc_bn254_random.h": ("gpbc_random_version", 1), "gpbc_bn254_forest.h": ("gpbc_forest_version", 1), "gpbc_bn254_mask.h": ("gpbc_mask_version", 1),
    "gpbc_bn254_verify.h": ("gpbc_verify_version", 1), "gpbc_bn254_member.h": ("gpbc_member_version", 1), "gpbc_bn254_gtfixed.h": ("gpbc_gtfixed_version", 1),
    "gpbc_bn254_openings.h": ("gpbc_openings_version", 1),
}


@pytest.fixture(scope="module")
def lib():
    _build.build_library()
    return _lib.load()


def included(header):
    """the project headers a public header includes, directly or through another one (recon.h and forest.h reach the main header through
    share.h, whose types they use)"""
    seen, todo = set(), [header]
    while todo:
        for name in re.findall(r'^#include "(gpbc_bn254\w*\.h)"', abi_headers.header_text(todo.pop()), flags=re.M):
            if name not in seen:
                seen.add(name)
                todo.append(name)
    return seen


@pytest.mark.parametrize("header", list(_lib.HEADERS))
def test_table_is_its_header_and_loaded(lib, header):
    """Every prototype of the header, return and parameter by parameter, is what its table declares, and load() has given every symbol
    its restype and argtypes from it: no call relies on ctypes' default of a 32-bit int."""
    table, protos = _lib.HEADERS[header], abi_headers.prototypes(header)
    assert sorted(protos) == abi_headers.declared_symbols(header) == sorted(table) and protos
    for name, (ret, params) in protos.items():
        assert table[name] == ret + ":" + "".join(params), name
        fn = getattr(lib, name)
        assert fn.restype is _lib._CTYPES[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [_lib._CTYPES[k] for k in params], name
    assert header == MAIN or MAIN in included(header)
    entry, value = VERSIONS[header]
    assert table[entry] == "i:" and getattr(lib, entry)() == value


def test_tables_cover_the_headers_and_the_library_exactly(lib):
    """a header without a line in _lib.HEADERS, a symbol in two tables, an export no table declares or a declared symbol the library lacks"""
    assert list(VERSIONS) == list(_lib.HEADERS) and list(_lib.HEADERS)[0] == MAIN
    on_disk = {os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "include", "gpbc_bn254*.h"))}
    assert set(_lib.HEADERS) == on_disk
    names = [name for table in _lib.HEADERS.values() for name in table]
    assert len(names) == len(set(names))                                                   # pairwise disjoint
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"^[0-9a-f]+ T (gpbc_\w+)$", nm, flags=re.M))
    assert set(names) == exported, (sorted(set(names) - exported), sorted(exported - set(names)))
    assert [n for table in _lib.HEADERS.values() for n, sig in table.items() if sig.startswith("s")] == ["gpbc_last_error"]
    assert _lib.EXPORTS == list(_lib.SIGNATURES) and _lib.HEADERS[MAIN] is _lib.SIGNATURES


def test_build_lists_are_the_files_of_csrc():
    csrc = lambda pattern: sorted(os.path.basename(f) for f in glob.glob(os.path.join(_build.CSRC, pattern)))
    assert sorted(_build.UNITS) == csrc("*.hip") and len(set(_build.UNITS)) == len(_build.UNITS)
    assert sorted(_build.HEADERS) == csrc("*.hpp") and len(set(_build.HEADERS)) == len(_build.HEADERS)
    deps = [os.path.realpath(d) for d in _build.dependencies()]
    assert len(set(deps)) == len(deps) and all(os.path.isfile(d) for d in deps)
    want = [os.path.join(_build.CSRC, f) for f in _build.UNITS + _build.HEADERS] + [os.path.join(ROOT, "include", h) for h in _lib.HEADERS]
    want.append(os.path.join(ROOT, "tools", "concurrent_calls.cpp"))
    assert set(deps) == {os.path.realpath(w) for w in want}


def test_isa_fence_scans_every_unit(tmp_path):
    """_check_isa refuses a unit it found no ISA file for, from the first unit to the last: a unit that is compiled is also scanned"""
    with pytest.raises(RuntimeError, match=re.escape(_build.UNITS[0])):
        _build._check_isa(str(tmp_path))
    for unit in _build.UNITS[:-1]:
        d = tmp_path / unit.replace(".hip", "")
        d.mkdir()
        (d / "x-gfx950.s").write_text("\tv_add_u32 v0, v1, v2\n")
    with pytest.raises(RuntimeError, match=re.escape(_build.UNITS[-1])):
        _build._check_isa(str(tmp_path))
    (tmp_path / _build.UNITS[-1].replace(".hip", "")).mkdir()
    (tmp_path / _build.UNITS[-1].replace(".hip", "") / "x-gfx950.s").write_text("\tv_add_u32 v0, v1, v2\n")
    _build._check_isa(str(tmp_path))                                                       # every unit scanned, nothing found
