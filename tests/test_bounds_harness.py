"""tests/bounds_harness.py against the harness it loads: HC_SIGNATURES is what the extern "C" blocks of tools/bounds_check.cpp define and
what the built library exports, and load() has declared every entry from it, so no call relies on ctypes' default of a 32-bit int."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT
import bounds_harness
from bounds_harness import CTYPES, HC_SIGNATURES, hc  # noqa: F401  (the fixture)


def defined_entries():
    """{symbol: "return kind:parameter kinds"} of every hc_* function defined inside an extern "C" block, parameter lists over several
    lines included"""
    text = open(os.path.join(ROOT, bounds_harness.SRC)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    blocks = []
    for m in re.finditer(r'^extern "C" \{', text, flags=re.M):                             # each block up to the brace that closes it
        depth, at = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(text[at], 0)
            at += 1
        blocks.append(text[m.end():at - 1])

    def kind(decl):
        if "*" in decl:
            return "p"
        words = set(re.findall(r"[A-Za-z_]\w*", decl))
        hits = [k for k, w in (("z", "size_t"), ("q", "uint64_t"), ("i", "int"), ("d", "double")) if w in words]
        assert len(hits) == 1, decl
        return hits[0]
    entries = {}
    for ret, name, params in re.findall(r"^(void|int|double)\s+(hc_\w+)\s*\(([^)]*)\)\s*\{", "\n".join(blocks), flags=re.M):
        assert name not in entries, name
        params = " ".join(params.split())
        entries[name] = {"void": "v", "int": "i", "double": "d"}[ret] + ":" + "".join([] if params in ("", "void") else [kind(p) for p in params.split(",")])
    return entries


def test_signature_table_is_the_source():
    entries = defined_entries()
    assert list(HC_SIGNATURES.items()) == list(entries.items())                            # names, kinds and the order of the file
    assert len(entries) >= 75 and {sig[0] for sig in entries.values()} == {"v", "i", "d"}
    assert {k for sig in entries.values() for k in sig[2:]} == {"p", "z", "i", "q"}
    assert "\n" in re.search(r"hc_fr_find_common\s*\(([^)]*)\)", open(os.path.join(ROOT, bounds_harness.SRC)).read()).group(1)   # a two-line list, parsed


def test_signature_table_is_the_library_and_loaded(hc):
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, bounds_harness.SO)], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"^[0-9a-f]+ T (hc_\w+)$", nm, flags=re.M)) == set(HC_SIGNATURES)
    for name, sig in HC_SIGNATURES.items():
        ret, params = sig.split(":")
        fn = getattr(hc, name)
        assert fn.restype is CTYPES[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [CTYPES[k] for k in params], name
    assert bounds_harness.load() is hc                                                     # one library per process
    assert not [f for f in os.listdir(os.path.join(ROOT, "tools")) if f.endswith(".tmp")]


def test_a_value_of_the_wrong_kind_is_refused(hc):
    assert HC_SIGNATURES["hc_subset_shape"] == "v:zzp"
    with pytest.raises(ctypes.ArgumentError):                                              # a double where the table says size_t
        hc.hc_subset_shape(ctypes.c_double(0), 1, None)
