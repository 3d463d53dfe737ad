"""LSSS matrices and 0 / 1 weights from boolean formulas on the device (run with -m gpu): gpbc_fr_lsss_from_formula and
gpbc_formula_select, host and _dev forms, on every case of tests/formula_cases.py against its recursive restatement, exactly, into caller
buffers with a guard row behind them; the device-built matrices and the masks through fr_lsss_weights, whose ok must agree item by item;
the refusals with a live device; the stream contract of both _dev entries (the gated procedure of tests/test_stream_contract_gpu.py)."""
import numpy as np
import pytest

import formula_cases as fc
from test_formula import build_mismatches, select_mismatches

pytestmark = pytest.mark.gpu
GUARD = 0xA5
BUILD, SELECT = fc.build_cases(), fc.select_cases()


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(eng, fn, inputs, sizes, tensors):
    """fn(*inputs, *outputs) into caller buffers one row longer than the results, filled with a guard byte; the results as host arrays"""
    import torch
    outs = [np.full(n + 64, GUARD, dtype=np.uint8) for n in sizes]
    if tensors:
        outs, inputs = [dev(b) for b in outs], [dev(a) for a in inputs]
    res = fn(*inputs, *[b[:n] for b, n in zip(outs, sizes)])
    if tensors:
        assert all(r.data_ptr() == b.data_ptr() for r, b in zip(res, outs))
        torch.cuda.synchronize()
        outs, res = [b.cpu().numpy() for b in outs], [r.cpu().numpy() for r in res]
    else:
        assert all(r.ctypes.data == b.ctypes.data for r, b in zip(res, outs))
    assert all((b[n:] == GUARD).all() for b, n in zip(outs, sizes))
    return res


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_from_formula_cases(eng, tensors):
    bad = []
    for c in BUILD:
        k, rows, cols = len(c["trees"]), c["rows"], c["cols"]
        got = guarded(eng, lambda nodes, *outs: eng.fr_lsss_from_formula(nodes, rows, cols, *outs), [c["nodes"]], [k * rows * cols * 32, k * rows * 8, k * 8, k], tensors)
        assert got[0].shape == (k, rows, cols, 32) and got[1].shape == (k, rows) and got[1].dtype == np.int64 and got[2].shape == (k, 2) and got[3].shape == (k,)
        bad += build_mismatches(c, got)
    assert bad == []


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_formula_select_cases(eng, tensors):
    bad = []
    for c in SELECT:
        k, rows = len(c["held"]), c["rows"]
        got = guarded(eng, lambda nodes, held, *outs: eng.formula_select(nodes, held.reshape(-1), rows, *outs), [c["nodes"], c["held"]], [k * rows, k], tensors)
        assert got[0].shape == (k, rows) and got[1].shape == (k,)
        bad += select_mismatches(c, got)
    assert bad == []


def test_an_unaligned_matrix_takes_the_byte_stores(eng):
    """a matrix_out that does not start on a 16-byte boundary: the same bytes, nothing outside"""
    import torch
    c = fc.by_label(BUILD, "up-to-4/wide")
    k, rows, cols = len(c["trees"]), c["rows"], c["cols"]
    buf = torch.full((k * rows * cols * 32 + 64,), GUARD, dtype=torch.uint8, device="cuda")
    got = eng.fr_lsss_from_formula(dev(c["nodes"]), rows, cols, matrix_out=buf[5:5 + k * rows * cols * 32])
    assert got[0].data_ptr() % 16 == 5
    torch.cuda.synchronize()
    assert build_mismatches(c, [g.cpu().numpy() for g in got]) == []
    host = buf.cpu().numpy()
    assert (host[:5] == GUARD).all() and (host[5 + k * rows * cols * 32:] == GUARD).all()


def test_ok_is_the_ok_of_the_field_solve_on_the_built_matrix(eng):
    """the matrices of fr_lsss_from_formula and the masks go through fr_lsss_weights: its ok is formula_select's, item by item, and its
    weights on the chosen-only mask are exactly the chosen rows with weight 1"""
    import torch
    one = np.frombuffer((1).to_bytes(32, "little"), dtype=np.uint8)
    for c in SELECT:
        k, rows = len(c["held"]), c["rows"]
        nodes, held = dev(c["nodes"]), dev(c["held"])
        matrix, rho, dims, built = eng.fr_lsss_from_formula(nodes, rows, 64)
        chosen, ok = eng.formula_select(nodes, held.reshape(-1), rows)
        w, solved = eng.fr_lsss_weights(matrix.reshape(-1), rows, 64, held.reshape(-1))
        again, solved_again = eng.fr_lsss_weights(matrix.reshape(-1), rows, 64, chosen.reshape(-1))
        torch.cuda.synchronize()
        ok, solved = ok.cpu().numpy(), solved.cpu().numpy()
        assert ok.tolist() == solved.tolist() == solved_again.cpu().numpy().tolist() == fc.expected_select(c)[1].tolist(), c["label"]
        want = chosen.cpu().numpy()[:, :, None] * one[None, None, :]
        assert again.cpu().numpy().reshape(k, rows, 32).tobytes() == want.tobytes(), c["label"]


def test_live_refusals_leave_the_buffers_untouched(eng):
    """GPBC_ERR_INVALID_ARG before any launch, nothing written: null pointers, sizes, overlapping buffers, too many items; k = 0 is a no-op"""
    import torch
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    hbuf = np.zeros(4096, dtype=np.uint8)
    for host, base in ((True, hbuf.ctypes.data + (-hbuf.ctypes.data) % 16), (False, buf.data_ptr())):
        extra = [] if host else [None]
        N, M, Rh, D, O, H, C = base, base + 256, base + 1024, base + 1280, base + 1408, base + 1536, base + 1664
        good = [N, 3, 2, 2, 2, M, Rh, D, O]                                                    # two formulas of three nodes, 2 x 2
        bad = [(0, None, b"null"), (5, None, b"null"), (6, None, b"null"), (8, None, b"null"), (1, 0, b"n_nodes"), (1, 128, b"n_nodes"), (3, 65, b"1 .. 64"),
               (4, 0, b"1 .. 64"), (2, 1 << 29, b"too many"), (5, N + 40, b"overlaps"), (6, M + 248, b"overlaps"), (7, Rh + 24, b"overlaps"), (8, D + 15, b"overlaps")]
        fn = lib.gpbc_fr_lsss_from_formula if host else lib.gpbc_fr_lsss_from_formula_dev
        for at, v, why in bad:
            args = list(good)
            args[at] = v
            assert fn(*args, *extra) == -1 and why in lib.gpbc_last_error(), (at, v, lib.gpbc_last_error())
        zero = list(good)
        zero[2] = 0
        assert fn(*zero, *extra) == 0
        good = [N, 1, 3, H, 4, 2, C, O]                                                        # one formula, four masks of two rows
        bad = [(0, None, b"null"), (3, None, b"null"), (6, None, b"null"), (7, None, b"null"), (1, 3, b"n_formulas"), (2, 128, b"n_nodes"), (5, 65, b"1 .. 64"),
               (4, 1 << 29, b"too many"), (6, H + 7, b"overlaps"), (6, N + 16, b"overlaps"), (7, H, b"overlaps"), (7, C + 7, b"overlaps")]
        fn = lib.gpbc_formula_select if host else lib.gpbc_formula_select_dev
        for at, v, why in bad:
            args = list(good)
            args[at] = v
            assert fn(*args, *extra) == -1 and why in lib.gpbc_last_error(), (at, v, lib.gpbc_last_error())
        zero = list(good)
        zero[4] = 0
        assert fn(*zero, *extra) == 0
    torch.cuda.synchronize()
    assert not buf.any().item() and not hbuf.any()
    nodes = dev(np.array([[fc.OR, 1, 2]], dtype=np.int64))
    with pytest.raises(ValueError, match="overlaps"):
        eng.fr_lsss_from_formula(nodes, 2, 1, matrix_out=buf[:64], ok_out=buf[63:64])
    with pytest.raises(ValueError, match="all be CUDA tensors or all host"):
        eng.formula_select(nodes, hbuf[:2], 2)
    assert tuple(eng.formula_select(nodes, buf[:0], 2)[0].shape) == (0, 2)
    torch.cuda.synchronize()
    assert not buf.any().item()


def test_dev_forms_are_ordered_on_the_callers_stream_and_do_not_wait(eng):
    """the gated procedure of tests/test_stream_contract_gpu.py: the results are those of the real inputs copied in behind a closed gate,
    and the calls return while the gate is closed"""
    import test_stream_contract_gpu as contract
    rig = contract.Rig(eng)
    three = np.ascontiguousarray(fc.by_label(BUILD, "up-to-4")["nodes"][3:11])                      # the eight formulas of three leaves
    sub = fc.by_label(SELECT, "ragged/64")
    shared = fc.by_label(SELECT, "shared/k130")
    case_list = [
        ("from_formula", lambda nodes: eng.fr_lsss_from_formula(nodes, 4, 4), (three,), None),
        ("formula_select", lambda nodes, held: eng.formula_select(nodes, held.reshape(-1), 64), (np.ascontiguousarray(sub["nodes"][20:40]), np.ascontiguousarray(sub["held"][20:40])), None),
        ("formula_select one formula", lambda nodes, held: eng.formula_select(nodes, held.reshape(-1), 6), (shared["nodes"], np.ascontiguousarray(shared["held"][:70])), None),
    ]
    wrong = contract.run_family(rig, "formulas", case_list)
    assert not wrong, "\n".join(wrong)
    assert {"gpbc_fr_lsss_from_formula_dev", "gpbc_formula_select_dev"} <= rig.seen
