"""The public headers under include/ as the tests read them: the one parser every ABI test shares (not collected: no test_ prefix)."""
import os
import re

from conftest import ROOT


def header_text(header_name):
    with open(os.path.join(ROOT, "include", header_name)) as f:
        return f.read()


def declared_symbols(header_name):
    """the sorted gpbc_* names followed by `(` outside the block comments of the header"""
    text = re.sub(r"/\*.*?\*/", "", header_text(header_name), flags=re.S)
    return sorted(set(re.findall(r"\b(gpbc_[a-z0-9_]+)\s*\(", text)))


def prototypes(header_name):
    """{symbol: (return kind, [parameter kinds])} parsed from the header, in the kinds of _lib.SIGNATURES: p for any type with a `*`,
    z size_t, l long, i int; s for a `const char *` return"""
    text = re.sub(r"/\*.*?\*/", "", header_text(header_name), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)

    def kind(decl, ret=False):
        if "*" in decl:
            assert not ret or re.fullmatch(r"\s*const\s+char\s*\*\s*", decl), decl
            return "s" if ret else "p"
        words = set(re.findall(r"[A-Za-z_]\w*", decl))
        hits = [k for k, w in (("z", "size_t"), ("l", "long"), ("i", "int")) if w in words]
        assert len(hits) == 1, decl
        return hits[0]
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\n\*]*?)\b(gpbc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        assert name not in protos, name
        params = " ".join(params.split())
        protos[name] = (kind(ret, ret=True), [] if params in ("", "void") else [kind(p) for p in params.split(",")])
    return protos
