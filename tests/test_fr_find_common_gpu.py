"""The common attributes of a list and a set on the device (run with -m gpu): gpbc_fr_find_common, host and _dev forms, on every case of
tests/select_cases.py against utils/find_common_attributes.go restated in Python integers, exactly, into caller buffers with a guard row
behind them; the `common` rows as the node sets of fr_lagrange_basis; the refusals with a live device; the stream contract of the _dev
entry (the gated procedure of tests/test_stream_contract_gpu.py) with a shared set and with a list of more than one chunk."""
import numpy as np
import pytest

import fr_lagrange_cases as lc
import select_cases as sel

pytestmark = pytest.mark.gpu
R = sel.R
GUARD = 0xA5


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded_call(eng, c, tensors):
    """fr_find_common into caller buffers one row longer than the results, filled with a guard byte"""
    import torch
    k, d = c["k"], c["d"]
    bufs = [np.full((k * d + 1) * 4, GUARD, dtype=np.uint8), np.full((k * d + 1) * 4, GUARD, dtype=np.uint8), np.full((k * d + 1) * 32, GUARD, dtype=np.uint8),
            np.full(k + 8, GUARD, dtype=np.uint8)]
    ends = [k * d * 4, k * d * 4, k * d * 32, k]
    S, L = sel.set_rows(c).reshape(-1), sel.list_rows(c).reshape(-1)
    if tensors:
        bufs = [dev(b) for b in bufs]
        S, L = dev(S), dev(L)
    res = eng.fr_find_common(S, L, c["m"], c["a"], d, *[b[:e] for b, e in zip(bufs, ends)])
    if tensors:
        assert all(r.data_ptr() == b.data_ptr() for r, b in zip(res, bufs)) and res[0].dtype == torch.int32
        torch.cuda.synchronize()
        bufs, res = [b.cpu().numpy() for b in bufs], [r.cpu().numpy() for r in res]
    else:
        assert all(r.ctypes.data == b.ctypes.data for r, b in zip(res, bufs)) and res[0].dtype == np.int32
    assert all((b[e:] == GUARD).all() for b, e in zip(bufs, ends)), c["label"]
    assert res[0].shape == res[1].shape == (k, d) and res[2].shape == (k, d, 32) and res[3].shape == (k,)
    return res


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_select_cases(eng, tensors):
    bad = []
    for c in sel.cases():
        bad += sel.mismatches(c, guarded_call(eng, c, tensors))
    assert bad == []


def test_common_rows_are_lagrange_sets(eng):
    """`common` goes into fr_lagrange_basis as it is: the coefficients at 0 over the kept attributes, against Python integers"""
    for label in ("a24-m32-k65-shared", "a24-m32-k65-own", "chunked", "named-values"):
        c = sel.by_label(label)
        d = c["d"]
        sp, lp, common, ok = eng.fr_find_common(dev(sel.set_rows(c).reshape(-1)), dev(sel.list_rows(c).reshape(-1)), c["m"], c["a"], d)
        delta = eng.fr_lagrange_basis(common.reshape(-1), d).cpu().numpy().reshape(c["k"], d, 32)
        ok = ok.cpu().numpy()
        assert ok.any(), label
        for j in np.nonzero(ok)[0]:
            kept = [t[2] for t in sel.expected_item(sel.item_set(c, j), c["lists"][j], d)]
            got = [int.from_bytes(r.tobytes(), "little") for r in delta[j]]
            assert got == [lc.basis(kept, i, 0) for i in kept], (label, j)


def test_live_refusals_leave_the_buffers_untouched(eng):
    """GPBC_ERR_INVALID_ARG before any launch, nothing written: null pointers, sizes, overlapping buffers, too many items; k = 0 is a no-op"""
    import torch
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    hbuf = np.zeros(64 * 32, dtype=np.uint8)
    for fn, base, extra in ((lib.gpbc_fr_find_common, hbuf.ctypes.data, []), (lib.gpbc_fr_find_common_dev, buf.data_ptr(), [None])):
        S, L, sp, lp, cm, ok = base, base + 128, base + 512, base + 576, base + 640, base + 1024      # m = 4, a = 3, d = 2, k = 4
        good = [S, 1, 4, L, 3, 2, 4, sp, lp, cm, ok]
        bad = [(0, None, b"null"), (3, None, b"null"), (7, None, b"null"), (8, None, b"null"), (9, None, b"null"), (10, None, b"null"),
               (1, 2, b"n_sets"), (2, 0, b"1 .. 1024"), (4, 1025, b"1 .. 1024"), (5, 0, b"1 .. 1024"), (6, 1 << 29, b"too many"),
               (7, S + 124, b"overlaps"), (8, sp + 28, b"overlaps"), (9, L + 380, b"overlaps"), (10, cm + 255, b"overlaps"), (10, lp, b"overlaps")]
        for at, v, why in bad:
            args = list(good)
            args[at] = v
            assert fn(*args, *extra) == -1 and why in lib.gpbc_last_error(), (at, v, lib.gpbc_last_error())
        zero = list(good)
        zero[6] = 0
        assert fn(*zero, *extra) == 0
    torch.cuda.synchronize()
    assert not buf.any().item() and not hbuf.any()
    with pytest.raises(ValueError, match="overlaps"):
        eng.fr_find_common(buf[:128], buf[128:512], 4, 3, 2, common_out=buf[256:512])
    with pytest.raises(ValueError, match="all be CUDA tensors or all host"):
        eng.fr_find_common(buf[:128], hbuf[128:512], 4, 3, 2)
    assert tuple(eng.fr_find_common(buf[:128], buf[:0], 4, 3, 2)[2].shape) == (0, 2, 32)
    torch.cuda.synchronize()
    assert not buf.any().item()


def test_dev_form_is_ordered_on_the_callers_stream_and_does_not_wait(eng):
    """the gated procedure of tests/test_stream_contract_gpu.py with a set for all items and with per-item sets and a list of three chunks:
    the results are those of the real inputs copied in behind a closed gate, and the call returns while the gate is closed"""
    import test_stream_contract_gpu as contract
    rig = contract.Rig(eng)
    case_list = []
    for label, name, items in (("find_common shared set", "a24-m32-k65-shared", 5), ("find_common chunks", "chunked", 3)):
        c = sel.by_label(name)
        m, a, d = c["m"], c["a"], c["d"]
        fn = (lambda m, a, d: lambda S, L: eng.fr_find_common(S.reshape(-1), L.reshape(-1), m, a, d))(m, a, d)
        S = sel.set_rows(c).reshape(-1, 32) if c["shared"] else sel.set_rows(c).reshape(c["k"], m * 32)[:items]
        case_list.append((label, fn, (np.ascontiguousarray(S), np.ascontiguousarray(sel.list_rows(c).reshape(c["k"], a * 32)[:items])), None))
    wrong = contract.run_family(rig, "find common", case_list)
    assert not wrong, "\n".join(wrong)
    assert "gpbc_fr_find_common_dev" in rig.seen
