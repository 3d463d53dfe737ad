"""IsOnCurve / IsInSubGroup of in-memory G1, G2 and GT elements on the MI355X (run with -m gpu): k_g1_is_on_curve, k_g2_is_on_curve,
k_g2_is_in_subgroup and k_gt_is_in_subgroup through bn254.py and the C entries, every verdict against the oracle's truth of
tests/member_cases.py (never against the code under test):

  * every case of the three corpora through the host form and the _dev form;
  * sizes at the wavefront edges — points n in {1, 63, 64, 65}, GT n in {1, 2, 31, 32, 33, 65} (32 elements per wavefront) — with good
    and bad elements mixed inside every wavefront;
  * one bad element among 31 good, one good among 31 bad, and an all-bad wavefront beside mixed ones in one call: the wavefront skip of
    the GT kernel must change no verdict;
  * a caller's `out` with guards round it, rows that are only 4-byte aligned, n = 0, GPBC_ERR_INVALID_ARG on an overlap;
  * a call on a non-default stream, gated as in tests/test_stream_contract_gpu.py: the entry reads its input behind the earlier work of
    that stream and returns without waiting for it;
  * cross-checks against existing entries: gt_equal(gt_exp(z, r), one) for canonical non-zero z, and g2_unmarshal(g2_marshal(Q)) for
    points Q on the twist."""
import numpy as np
import pytest

import bn254_py as o
import member_cases as mc

pytestmark = pytest.mark.gpu
GUARD = 0xA5

# entry -> (corpus, truth)
ENTRIES = {"g1_is_on_curve": (mc.g1_cases, "on_curve"), "g2_is_on_curve": (mc.g2_cases, "on_curve"), "g2_is_in_subgroup": (mc.g2_cases, "in_subgroup"),
           "gt_is_in_subgroup": (mc.gt_cases, "in_subgroup")}
POINT_SIZES, GT_SIZES = (1, 63, 64, 65), (1, 2, 31, 32, 33, 65)


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def both_forms(eng, entry, data, want, what):
    """the host form and the _dev form on the same rows, each against the truth"""
    import torch
    fn = getattr(eng, entry)
    host = fn(data)
    assert isinstance(host, np.ndarray) and host.dtype == np.uint8 and host.shape == want.shape
    assert host.tolist() == want.tolist(), (entry, what, "host", np.nonzero(host != want)[0].tolist())
    dev = fn(to_dev(data))
    assert dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == want.shape
    got = dev.cpu().numpy()
    assert got.tolist() == want.tolist(), (entry, what, "device", np.nonzero(got != want)[0].tolist())


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_case_host_and_device(eng, entry):
    corpus, truth = ENTRIES[entry][0](), ENTRIES[entry][1]
    fn = getattr(eng, entry)
    want = corpus.truth[truth]
    for form, got in (("host", fn(corpus.data)), ("device", fn(to_dev(corpus.data)).cpu().numpy())):
        assert got.tolist() == want.tolist(), (entry, form, [(corpus.describe(i), int(got[i])) for i in np.nonzero(got != want)[0]])
    assert 0 < int(want.sum()) < len(want)
    if entry == "g1_is_on_curve":
        assert eng.g1_is_in_subgroup(corpus.data).tolist() == want.tolist()                # the alias


@pytest.mark.parametrize("entry,n", [(e, n) for e in ENTRIES for n in (GT_SIZES if e.startswith("gt") else POINT_SIZES)])
def test_sizes_at_the_wavefront_edges(eng, entry, n):
    corpus, truth = ENTRIES[entry][0](), ENTRIES[entry][1]
    data, want, _ = mc.tiled(corpus, n, truth, "mixed")
    both_forms(eng, entry, data, want, "mixed n = %d" % n)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_one_bad_one_good_and_an_all_bad_wavefront(eng, entry):
    """every wavefront of the first call holds one bad element, of the second one good element; the third call puts a wavefront of bad
    elements only — which the GT kernel skips — in front of, between and behind mixed ones"""
    corpus, truth = ENTRIES[entry][0](), ENTRIES[entry][1]
    block = 32 if entry.startswith("gt") else 64
    for pattern in ("one_bad", "one_good"):
        data, want, _ = mc.tiled(corpus, 2 * block + 1, truth, pattern)
        assert int((want[:block] == (pattern == "one_good")).sum()) == 1
        both_forms(eng, entry, data, want, pattern)
    bad, bad_want, _ = mc.tiled(corpus, block, truth, "all_bad")
    mix, mix_want, _ = mc.tiled(corpus, block + 1, truth, "mixed")
    assert not bad_want.any() and 0 < int(mix_want[:block].sum()) < block
    data = np.concatenate([bad, mix[:block], bad, mix])
    both_forms(eng, entry, data, np.concatenate([bad_want, mix_want[:block], bad_want, mix_want]), "all-bad wavefronts among mixed ones")
    both_forms(eng, entry, bad, bad_want, "one all-bad wavefront alone")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_caller_out_alignment_empty_and_overlap(eng, entry):
    import torch
    from gopairingbasedcryptography_amd import EngineError
    corpus, truth = ENTRIES[entry][0](), ENTRIES[entry][1]
    fn, width = getattr(eng, entry), corpus.width
    n = 33
    data, want, _ = mc.tiled(corpus, n, truth, "mixed")
    # a caller's out on the device, guards on both sides
    buf = torch.full((n + 16,), GUARD, dtype=torch.uint8, device="cuda")
    out = fn(to_dev(data), out=buf[5:5 + n])
    assert out.data_ptr() == buf.data_ptr() + 5 and out.cpu().numpy().tolist() == want.tolist()
    assert bool((buf[:5] == GUARD).all()) and bool((buf[5 + n:] == GUARD).all())
    # ... and on the host
    h = np.full(n + 8, GUARD, dtype=np.uint8)
    assert fn(data, out=h[:n]).tolist() == want.tolist() and (h[n:] == GUARD).all()
    # rows that are only 4-byte aligned
    raw = torch.zeros(n * width + 16, dtype=torch.uint8, device="cuda")
    raw[4:4 + n * width] = to_dev(data).reshape(-1)
    assert fn(raw[4:4 + n * width]).cpu().numpy().tolist() == want.tolist()
    # n = 0
    assert fn(np.zeros((0, width), dtype=np.uint8)).shape == (0,)
    e = fn(torch.zeros((0, width), dtype=torch.uint8, device="cuda"))
    assert e.is_cuda and tuple(e.shape) == (0,)
    lib = eng._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    assert getattr(lib, "gpbc_" + entry)(None, 0, None) == 0 and getattr(lib, "gpbc_%s_dev" % entry)(None, 0, None, st) == 0
    # ok_out inside the input: refused by the C entry before any launch, the input left as it was
    d = to_dev(data)
    before = d.clone()
    with pytest.raises(EngineError, match="overlaps"):
        fn(d, out=d.reshape(-1)[n * width - n:])
    with pytest.raises(EngineError, match="overlaps"):
        fn(d, out=d.reshape(-1)[:n])
    hd = np.array(data, copy=True)
    with pytest.raises(EngineError, match="overlaps"):
        fn(hd, out=hd.reshape(-1)[8:8 + n])
    torch.cuda.synchronize()
    assert bool((d == before).all()) and (hd == data).all()
    with pytest.raises(ValueError):
        fn(d, out=np.zeros(n, dtype=np.uint8))                                            # a device input with a host out


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_call_on_a_non_default_stream(eng, entry):
    """On a side stream the argument tensor holds a DECOY with the opposite verdicts; then, all on that stream: a bounded device-side
    delay, a copy of the real rows over the argument, an event, the entry, a clone of its verdicts, the decoy back.  A kernel on another
    stream, or a read outside the stream's order, sees the decoy.  The event is still pending when the call returns: the entry does not
    wait for its stream."""
    import torch
    corpus, truth = ENTRIES[entry][0](), ENTRIES[entry][1]
    fn = getattr(eng, entry)
    n = 40
    t = corpus.truth[truth]
    good, bad = np.nonzero(t == 1)[0], np.nonzero(t == 0)[0]
    real_idx = np.array([(good if i % 3 else bad)[i % len(good if i % 3 else bad)] for i in range(n)])
    decoy_idx = np.array([(bad if i % 3 else good)[i % len(bad if i % 3 else good)] for i in range(n)])
    real, decoy, want = to_dev(corpus.data[real_idx]), to_dev(corpus.data[decoy_idx]), t[real_idx]
    assert (t[decoy_idx] != want).all()
    fn(real)                                                                               # (the first call pays the kernel's load)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    arg = decoy.clone()
    filled = torch.cuda.Event()
    gated = hasattr(torch.cuda, "_sleep")
    if gated:                                                                              # sleep cycles per millisecond, measured
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(10 ** 5)
        e0.record()
        torch.cuda._sleep(10 ** 6)
        e1.record()
        e1.synchronize()
        gate_cycles = int(min(30.0 * 1e6 / max(e0.elapsed_time(e1), 1e-3), 3e8))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        if gated:
            torch.cuda._sleep(gate_cycles)                                                 # about 30 ms, bounded by construction
        arg.copy_(real, non_blocking=True)
        filled.record(side)
        out = fn(arg)
        returned_before_the_gate_opened = not filled.query()
        got = out.clone()
        arg.copy_(decoy, non_blocking=True)
    side.synchronize()
    assert got.cpu().numpy().tolist() == want.tolist()
    assert returned_before_the_gate_opened or not gated
    torch.cuda.synchronize()


def test_gt_verdict_equals_exponentiation_by_r(eng):
    """the only route the entries before this one offer: gt_equal(gt_exp(z, r), one), a 256-bit generic exponentiation — on canonical
    non-zero elements it is the same verdict"""
    c = mc.gt_cases()
    pick = [i for cls in ("one", "pairing", "pairing_power", "pairing_inverse", "easy_part_only", "pairing_times_easy", "random", "miller", "minus_one",
                          "minus_pairing", "one_limb_changed") for i in c.of(cls)[:2]]
    z = c.data[pick]
    assert all(mc.canonical(bytes(r)) and r.any() for r in z)
    one = np.frombuffer(o.gt_to_bytes(o.F12_ONE), dtype=np.uint8)
    by_exp = eng.gt_equal(eng.gt_exp(z, [o.R] * len(pick)), one)
    got = eng.gt_is_in_subgroup(z)
    assert got.tolist() == by_exp.tolist() == c.truth["in_subgroup"][pick].tolist() and 0 < int(got.sum()) < len(pick)


def test_g2_verdict_equals_marshal_then_unmarshal(eng):
    """g2_unmarshal(g2_marshal(Q)) accepts exactly the points of the twist that g2_is_in_subgroup accepts"""
    c = mc.g2_cases()
    pick = [i for cls in ("subgroup", "generator_multiple", "infinity", "off_subgroup", "cofactor_group", "order_10069", "subgroup_plus_cofactor", "y2_in_fp")
            for i in c.of(cls)[:3]]
    Q = c.data[pick]
    assert c.truth["on_curve"][pick].all()
    for compressed in (False, True):
        rows, ok = eng.g2_unmarshal(eng.g2_marshal(Q, compressed=compressed), 64 if compressed else 128)
        got = eng.g2_is_in_subgroup(Q)
        assert np.asarray(ok).tolist() == got.tolist() == c.truth["in_subgroup"][pick].tolist(), compressed
        assert all(rows[i].tobytes() == Q[i].tobytes() for i in range(len(pick)) if got[i])
    assert 0 < int(got.sum()) < len(pick)
