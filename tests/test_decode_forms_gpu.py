"""Unmarshal, marshal and map to curve on the edge corpus of tests/wire_cases.py, through EVERY kernel form (run with -m gpu on an MI355X).
The host code picks a kernel by call size (csrc/gpbc_wire.hip: one element per octet of lanes, per quad, per lane); each form of the G2
subgroup test and of the cofactor clearing is a chain of lane-crossing point arithmetic of its own.  One corpus — refusals of every kind
next to accepted rows, special field elements next to random ones — goes through a call of every size class, tiled so that wavefronts mix
outcomes ("shuffled") or take one path as a whole ("runs"), on the device entries (torch tensors) and the host entries (numpy arrays),
against the big-integer oracle bit for bit.  The kernel each device call ran is read back from the launch profile and compared with the
form the size is meant to reach, so a moved threshold fails here instead of silently ending the coverage of a form."""
import ctypes
import os
import re

import numpy as np
import pytest

import wire_cases as wc

pytestmark = pytest.mark.gpu

# n of the device-entry calls and the form each is meant to run
G2_DECODE_SIZES = ((1, "oct"), (7, "oct"), (2047, "oct"), (2048, "oct"), (2049, "quad"), (16384, "quad"), (16385, "lane"), (20011, "lane"))
ONE_KERNEL_SIZES = (1, 2049, 16385)                                   # G1 / GT unmarshal, every marshal: one kernel each
HOST_SIZES = (24, 2049, 20011)
G1_MAP_SIZES = ((6, "quad"), (16384, "quad"), (16385, "lane"))
G2_MAP_SIZES = ((4, "oct"), (2048, "oct"), (2049, "quad"), (16384, "quad"), (16385, "lane"))
KERNELS = {"g2_decode": {"oct": "k_g2_decode_oct", "quad": "k_g2_decode_quad", "lane": "k_g2_decode"},
           "g2_map": {"oct": "k_g2_map_fields_oct", "quad": "k_g2_map_fields_quad", "lane": "k_g2_map_fields"},
           "g1_map": {"quad": "k_g1_map_fields_quad", "lane": "k_g1_map_fields"},
           "g1_decode": "k_g1_decode", "gt_decode": "k_gt_decode", "g1_encode": "k_g1_encode", "g2_encode": "k_g2_encode"}
DECODE_SETS = (("g1", 32), ("g1", 64), ("g2", 64), ("g2", 128), ("gt", 384))
MEM_W = {"g1": 64, "g2": 128, "gt": 384}


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def _limits():
    """the size limits of the forms, from the source the library was built from"""
    from gopairingbasedcryptography_amd import _lib
    with open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "gpbc_wire.hip")) as f:
        src = f.read()
    lim = {k: int(v) for k, v in re.findall(r"constexpr size_t (WIRE_OCT_MAX|WIRE_QUAD_MAX|H2C_OCT_MAX|H2C_QUAD_MAX) = (\d+);", src)}
    assert len(lim) == 4, lim
    return lim


def _form(n, oct_max, quad_max):
    return "oct" if oct_max is not None and n <= oct_max else "quad" if n <= quad_max else "lane"


def test_every_size_reaches_the_form_it_is_meant_to():
    """The sizes above against the limits in csrc/gpbc_wire.hip: each form of each entry is reached on both sides of its limits.  (Which
    kernel a call really ran is asserted call by call below.)"""
    lim = _limits()
    for n, form in G2_DECODE_SIZES:
        assert _form(n, lim["WIRE_OCT_MAX"], lim["WIRE_QUAD_MAX"]) == form, ("G2 unmarshal", n, lim)
    for n, form in G2_MAP_SIZES:
        assert _form(n, lim["H2C_OCT_MAX"], lim["H2C_QUAD_MAX"]) == form, ("G2 map", n, lim)
    for n, form in G1_MAP_SIZES:
        assert _form(n, None, lim["H2C_QUAD_MAX"]) == form, ("G1 map", n, lim)
    for sizes, lo, hi in ((G2_DECODE_SIZES, "WIRE_OCT_MAX", "WIRE_QUAD_MAX"), (G2_MAP_SIZES, "H2C_OCT_MAX", "H2C_QUAD_MAX")):
        ns = [n for n, _ in sizes]
        assert {lim[lo], lim[lo] + 1, lim[hi], lim[hi] + 1} <= set(ns), (ns, lim)


def _profiled(eng, fn):
    """fn() and the names of the kernels it launched"""
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    _lib.check(lib.gpbc_profile_begin(eng._torch_stream()))
    out = fn()
    names, ms, cnt, nk = ctypes.create_string_buffer(32 * 16), (ctypes.c_double * 16)(), (ctypes.c_int * 16)(), ctypes.c_int(0)
    _lib.check(lib.gpbc_profile_end(names, ms, cnt, 16, ctypes.byref(nk)))
    return out, [names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode() for i in range(nk.value)]


def _decode_corpus(kind, slot):
    return wc.gt_decode_cases() if kind == "gt" else wc.decode_cases(kind, slot)


def _unmarshal(eng, kind, buf, slot):
    return eng.gt_unmarshal(buf) if kind == "gt" else getattr(eng, kind + "_unmarshal")(buf, elem_bytes=slot)


def _decode_sizes(kind):
    if kind == "g2":
        return [(n, form, KERNELS["g2_decode"][form]) for n, form in G2_DECODE_SIZES]
    return [(n, "lane", KERNELS[kind + "_decode"]) for n in ONE_KERNEL_SIZES]


@pytest.mark.parametrize("arrangement", wc.ARRANGEMENTS)
@pytest.mark.parametrize("kind,slot", DECODE_SETS)
def test_unmarshal_device_entry_every_form(eng, kind, slot, arrangement):
    import torch
    corpus = _decode_corpus(kind, slot)
    for n, form, kernel in _decode_sizes(kind):
        data, want_ok, want_rows, idx = wc.tiled(corpus, n, arrangement)
        buf = torch.from_numpy(data.reshape(-1)).cuda()
        (out, ok), names = _profiled(eng, lambda: _unmarshal(eng, kind, buf, slot))
        assert names == [kernel], (kind, slot, n, form, names)
        assert ok.dtype == torch.uint8 and tuple(ok.shape) == (n,) and tuple(out.shape) == (n, MEM_W[kind])
        ok, out = ok.cpu().numpy(), out.cpu().numpy()
        assert set(ok.tolist()) <= {0, 1}, (kind, slot, n, form)
        assert not wc.mismatches(corpus, idx, out, ok, want_rows, want_ok), (kind, slot, n, form, kernel, arrangement)


@pytest.mark.parametrize("arrangement", wc.ARRANGEMENTS)
@pytest.mark.parametrize("kind,slot", DECODE_SETS)
def test_unmarshal_host_entry(eng, kind, slot, arrangement):
    corpus = _decode_corpus(kind, slot)
    for n in HOST_SIZES:
        data, want_ok, want_rows, idx = wc.tiled(corpus, n, arrangement)
        out, ok = _unmarshal(eng, kind, data.reshape(-1), slot)
        assert ok.dtype == np.uint8 and ok.shape == (n,) and out.shape == (n, MEM_W[kind]) and set(ok.tolist()) <= {0, 1}, (kind, slot, n)
        assert not wc.mismatches(corpus, idx, out, ok, want_rows, want_ok), (kind, slot, n, arrangement)


def test_unmarshal_writes_nothing_behind_the_last_element(eng):
    """The raw device entries on buffers with one more output row and one more ok byte than the call has elements, at sizes that end inside
    a wavefront (the quad and octet kernels write from lane 0 of 4 or 8 lanes: a tail that wrote past n would land there).  The guard row
    and the guard byte keep their pattern; everything before them is the oracle's answer."""
    import torch
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    sizes = {"g2": (7, 2049, 16385), "g1": (1, 2049, 16385), "gt": (1, 2049, 16385)}
    elems_per_wave = {"oct": 8, "quad": 16, "lane": 64}
    for kind, slot in DECODE_SETS:
        corpus = _decode_corpus(kind, slot)
        by_n = {n: (form, kernel) for n, form, kernel in _decode_sizes(kind)}
        for n in sizes[kind]:
            form, kernel = by_n[n]
            assert n % elems_per_wave[form], (kind, n, form)
            data, want_ok, want_rows, idx = wc.tiled(corpus, n, "shuffled")
            buf = torch.from_numpy(data.reshape(-1)).cuda()
            out = torch.full((n + 1, MEM_W[kind]), 0xA5, dtype=torch.uint8, device="cuda")
            ok = torch.full((n + 1,), 0x5A, dtype=torch.uint8, device="cuda")
            eb = () if kind == "gt" else (ctypes.c_size_t(slot),)
            fn = getattr(lib, "gpbc_%s_unmarshal_batch_dev" % kind)
            _, names = _profiled(eng, lambda: _lib.check(fn(ctypes.c_void_p(buf.data_ptr()), *eb, ctypes.c_size_t(n), ctypes.c_void_p(out.data_ptr()),
                                                            ctypes.c_void_p(ok.data_ptr()), eng._torch_stream())))
            torch.cuda.synchronize()
            assert names == [kernel], (kind, slot, n, names)
            out, ok = out.cpu().numpy(), ok.cpu().numpy()
            assert (out[n] == 0xA5).all() and ok[n] == 0x5A, (kind, slot, n, form, "wrote behind the last element")
            assert not wc.mismatches(corpus, idx, out[:n], ok[:n], want_rows, want_ok), (kind, slot, n, form)


@pytest.mark.parametrize("kind,slot", (("g2", 64), ("g2", 128)))
def test_g2_unmarshal_forms_agree(eng, kind, slot):
    """The same rows through the octet, the quad and the per-lane kernel give the same answers (implied by the oracle comparison above;
    asserted on its own so that a failure names the form)."""
    import torch
    lim = _limits()
    corpus = wc.decode_cases(kind, slot)
    got = {}
    data, _, _, idx = wc.tiled(corpus, lim["WIRE_QUAD_MAX"] + 1, "shuffled")
    for n in (lim["WIRE_OCT_MAX"], lim["WIRE_OCT_MAX"] + 1, lim["WIRE_QUAD_MAX"] + 1):
        (out, ok), names = _profiled(eng, lambda: eng.g2_unmarshal(torch.from_numpy(data[:n].reshape(-1)).cuda(), elem_bytes=slot))
        got[names[0]] = (np.concatenate([out.cpu().numpy(), ok.cpu().numpy().reshape(-1, 1)], axis=1), idx[:n])
    assert sorted(got) == sorted(KERNELS["g2_decode"].values()), sorted(got)
    ref, ref_idx = got["k_g2_decode_oct"]
    assert len(corpus) <= len(ref_idx)
    by_case = np.zeros((len(corpus), ref.shape[1]), dtype=np.uint8)
    by_case[ref_idx] = ref                                             # (equal inputs of the octet call agree with each other: checked next)
    for name, (rows, idx) in got.items():
        bad = np.nonzero((rows != by_case[idx]).any(axis=1))[0]
        assert bad.size == 0, (name, "differs from k_g2_decode_oct", slot, [(int(j), corpus.describe(idx[j])) for j in bad[:6]])


@pytest.mark.parametrize("arrangement", wc.ARRANGEMENTS)
@pytest.mark.parametrize("kind", ("g1", "g2"))
def test_marshal_edge_points(eng, kind, arrangement):
    """Accepted points of the corpus, G1 points with y next to (p - 1) / 2 (decided in the lowest word of wire_words_lex_largest) and
    twist points whose y has a zero half (f2_lex_largest's a1 == 0 and a0 == 0 paths), both forms, device and host entry."""
    import torch
    marshal = getattr(eng, kind + "_marshal")
    for comp in (False, True):
        corpus = wc.marshal_cases(kind, comp)
        for n in ONE_KERNEL_SIZES:
            data, ok, want, idx = wc.tiled(corpus, n, arrangement)
            enc, names = _profiled(eng, lambda: marshal(torch.from_numpy(data.reshape(-1)).cuda(), compressed=comp))
            assert names == [KERNELS[kind + "_encode"]], (kind, comp, n, names)
            assert not wc.mismatches(corpus, idx, enc.cpu().numpy(), ok, want, ok), (kind, comp, n, arrangement, "device entry")
            if n == 2049:
                assert not wc.mismatches(corpus, idx, marshal(data.reshape(-1), compressed=comp), ok, want, ok), (kind, comp, n, arrangement, "host entry")


@pytest.mark.parametrize("arrangement", wc.ARRANGEMENTS)
@pytest.mark.parametrize("g2", (False, True))
def test_map_to_curve_every_form(eng, g2, arrangement):
    """The map corpus — u = 0, the exceptional u, p - 1, equal elements (the final addition doubles), opposite elements (infinity), and for
    G2 elements whose x1 has g(x1) in Fp — through the octet, quad and per-lane kernels, and through the host entry."""
    import torch
    corpus = wc.map_cases(g2)
    fn = eng.map_to_g2 if g2 else eng.map_to_g1
    kernels = KERNELS["g2_map" if g2 else "g1_map"]
    for n, form in (G2_MAP_SIZES if g2 else G1_MAP_SIZES):
        kernel = kernels[form]
        data, ok, want, idx = wc.tiled(corpus, n, arrangement)
        out, names = _profiled(eng, lambda: fn(torch.from_numpy(data.reshape(-1)).cuda()))
        assert names == [kernel], (g2, n, form, names)
        assert not wc.mismatches(corpus, idx, out.cpu().numpy(), ok, want, ok), (g2, n, form, kernel, arrangement)
    data, ok, want, idx = wc.tiled(corpus, 2049, arrangement)
    assert not wc.mismatches(corpus, idx, fn(data.reshape(-1)), ok, want, ok), (g2, 2049, arrangement, "host entry")


@pytest.mark.parametrize("g2", (False, True))
def test_map_to_curve_forms_agree(eng, g2):
    import torch
    lim = _limits()
    corpus = wc.map_cases(g2)
    fn = eng.map_to_g2 if g2 else eng.map_to_g1
    kernels = KERNELS["g2_map" if g2 else "g1_map"]
    data, _, _, idx = wc.tiled(corpus, lim["H2C_QUAD_MAX"] + 1, "shuffled")
    got = {}
    for n in (lim["H2C_OCT_MAX"], lim["H2C_OCT_MAX"] + 1, lim["H2C_QUAD_MAX"] + 1):
        out, names = _profiled(eng, lambda: fn(torch.from_numpy(data[:n].reshape(-1)).cuda()))
        got.setdefault(names[0], (out.cpu().numpy(), idx[:n]))
    assert sorted(got) == sorted(kernels.values()), sorted(got)
    first = "k_g2_map_fields_oct" if g2 else "k_g1_map_fields_quad"
    ref, ref_idx = got[first]
    by_case = np.zeros((len(corpus), ref.shape[1]), dtype=np.uint8)
    by_case[ref_idx] = ref
    for name, (rows, idx_n) in got.items():
        bad = np.nonzero((rows != by_case[idx_n]).any(axis=1))[0]
        assert bad.size == 0, (name, "differs from " + first, [(int(j), corpus.describe(idx_n[j])) for j in bad[:6]])
