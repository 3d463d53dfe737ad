"""Reconstruction weights of a threshold tree on the device (run with -m gpu): gpbc_fr_tree_weights, host and _dev forms, on every case
of tests/tree_weight_cases.py against bsw07.decrypt_plan in Python integers, byte for byte, into caller buffers with a guard row behind
them; the weights as device scalars against ShareTree.share's output (fr_mul and a sum give the secret back); the refusals of a live
handle; the stream contract of the _dev entry (the gated procedure of tests/test_stream_contract_gpu.py) at both LDS instances."""
import numpy as np
import pytest

import fr_cases as fc
import share_cases as sc
import tree_weight_cases as tw

pytestmark = pytest.mark.gpu
R = fc.R
GUARD = 0xA5


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


@pytest.fixture(scope="module")
def handles(eng):
    """one handle per tree of the case list"""
    made = {label: eng.ShareTree(sc.preorder(tree)) for label, tree, _ in tw.trees()}
    yield made
    for h in made.values():
        h.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded_call(handles, tensors):
    """weights() into caller buffers one row longer than the result, filled with a guard byte"""
    import torch

    def call(c):
        k, L = c["k"], c["L"]
        w, ok = np.full((k * L + 1, 32), GUARD, dtype=np.uint8), np.full(k + 1, GUARD, dtype=np.uint8)
        held = np.ascontiguousarray(c["held"]).reshape(-1)
        h = handles[c["label"].split("/")[0]]
        if tensors:
            w, ok = dev(w), dev(ok)
            rw, rok = h.weights(dev(held), out=w[:k * L], ok_out=ok[:k])
            assert rw.data_ptr() == w.data_ptr() and rok.data_ptr() == ok.data_ptr()
            torch.cuda.synchronize()
            w, ok = w.cpu().numpy(), ok.cpu().numpy()
        else:
            rw, rok = h.weights(held, out=w[:k * L], ok_out=ok[:k])
            assert rw.ctypes.data == w.ctypes.data and rok.ctypes.data == ok.ctypes.data
        assert (w[k * L] == GUARD).all() and ok[k] == GUARD, c["label"]
        return w[:k * L], ok[:k]
    return call


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_tree_weight_cases(handles, tensors):
    assert tw.run_cases(guarded_call(handles, tensors), tw.cases()) == []


def test_weights_recombine_the_shares_on_the_device(eng, handles):
    """share() of k secrets and weights() of k held sets on one handle, both left on the device: fr_mul of the two and a sum over the
    leaves give every satisfied item's secret back"""
    for label in ("example", "alternating", "3of5-2of3", "chain8", "16x16", "many-gates", "65-of-65"):
        c = next(c for c in tw.cases() if c["label"] == label)
        h, k, L = handles[label], c["k"], c["L"]
        secrets, coeffs = sc.rand("twg-s-" + label, k), sc.rand("twg-q-" + label, k * h.coeffs)
        shares = h.share(dev(fc.rows(secrets).reshape(-1)), dev(fc.rows(coeffs).reshape(-1)) if h.coeffs else None)
        w, ok = h.weights(dev(c["held"].reshape(-1)))
        prod = eng.fr_mul(w.reshape(-1), shares.reshape(-1)).reshape(k, L, 32)
        acc = prod[:, 0].contiguous()
        for y in range(1, L):
            acc = eng.fr_add(acc.reshape(-1), prod[:, y].contiguous().reshape(-1))
        got, ok = fc.ints(acc.cpu().numpy()), ok.cpu().numpy()
        assert ok.tolist() == tw.expected(c)[1] and ok.any(), label
        assert [g for g, o in zip(got, ok) if o] == [s % R for s, o in zip(secrets, ok) if o], label
        assert not any(g for g, o in zip(got, ok) if not o), label


def test_python_values_go_in_and_outputs_are_canonical(eng, handles):
    c = next(c for c in tw.cases() if c["label"] == "example")
    h = handles["example"]
    w, ok = h.weights([[bool(v) for v in row] for row in c["held"]])                  # nested bools
    assert (fc.ints(w), ok.tolist()) == tw.expected(c) and tuple(w.shape) == (c["k"], c["L"], 32)
    w2, _ = h.weights(c["held"] != 0)                                                 # a bool array
    assert (w2 == w).all()
    flat = w.reshape(-1)
    assert (eng.fr_add(flat, fc.rows([0]).reshape(-1)).reshape(-1) == flat).all() and max(fc.ints(w)) < R


def test_a_live_handle_refuses_what_the_header_says(eng, handles):
    """GPBC_ERR_INVALID_ARG before any launch, nothing written: null pointers, overlapping buffers, too many items; k = 0 is a no-op"""
    import torch
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    h = handles["2-of-3"]._h
    buf = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    hbuf = np.zeros(64 * 32, dtype=np.uint8)
    for fn, base, extra in ((lib.gpbc_fr_tree_weights, hbuf.ctypes.data, []), (lib.gpbc_fr_tree_weights_dev, buf.data_ptr(), [None])):
        held, w, ok = base, base + 64, base + 1024
        bad = [((None, 2, w, ok), b"null"), ((held, 2, None, ok), b"null"), ((held, 2, w, None), b"null"),
               ((held, 1 << 29, w, ok), b"too many items"), ((held, (1 << 64) - 1, w, ok), b"too many items"),
               ((held, 2, held + 5, ok), b"overlaps"), ((held, 2, w, held + 5), b"overlaps"), ((held, 2, w, w + 191), b"overlaps"), ((held + 64 + 191, 2, w, ok), b"overlaps")]
        for (a, k, b, c), why in bad:
            assert fn(h, a, k, b, c, *extra) == -1 and why in lib.gpbc_last_error(), (k, why, lib.gpbc_last_error())
        assert fn(h, None, 0, None, None, *extra) == 0
    torch.cuda.synchronize()
    assert not buf.any().item() and not hbuf.any()
    t = handles["2-of-3"]
    with pytest.raises(ValueError, match="overlaps"):
        t.weights(buf[:6], out=buf[:2 * 3 * 32])
    with pytest.raises(ValueError, match="whole items"):
        t.weights(buf[:7])
    assert tuple(t.weights(buf[:0])[0].shape) == (0, 3, 32)
    closed = eng.ShareTree(sc.preorder(sc.flat_gate(2, 3)))
    closed.close()
    with pytest.raises(ValueError, match="closed"):
        closed.weights(buf[:3])


def test_handle_of_another_device_is_refused(eng):
    """with two devices bound: a tree made on the first, tensors on the second"""
    import torch
    if eng.num_devices() < 2:
        pytest.skip("one device bound")
    from gopairingbasedcryptography_amd import EngineError
    first, second = sorted(eng._slots)[:2]
    with torch.cuda.device(first):
        eng._bind(torch.device("cuda", first))
        t = eng.ShareTree(sc.preorder(sc.flat_gate(2, 3)))
    held = torch.ones(3, dtype=torch.uint8, device="cuda:%d" % second)
    out = torch.zeros(3 * 32 + 1, dtype=torch.uint8, device="cuda:%d" % second)
    with pytest.raises(EngineError, match="created on device"):
        t.weights(held, out=out[:96], ok_out=out[96:])
    torch.cuda.synchronize(second)
    assert not out.any().item()
    t.close()


def test_one_handle_serves_both_directions_after_release(eng, handles):
    c = next(c for c in tw.cases() if c["label"] == "alternating")
    s = next(s for s in sc.tree_cases() if s["label"] == "alternating")
    h = handles["alternating"]
    want = tw.expected(c)
    for _ in range(2):
        w, ok = h.weights(c["held"].reshape(-1))
        assert (fc.ints(w), ok.tolist()) == want
        assert fc.ints(h.share(s["secrets"], s["coeffs"])) == sc.tree_expected(s)
        eng.release_workspaces()
    w, ok = h.weights(c["held"][:7].reshape(-1))                                       # another item count on the same handle
    assert fc.ints(w) == want[0][:7 * c["L"]] and ok.tolist() == want[1][:7]


def test_dev_form_is_ordered_on_the_callers_stream_and_does_not_wait(eng, handles):
    """the gated procedure of tests/test_stream_contract_gpu.py at both LDS instances: the results are those of the real held sets copied
    in behind a closed gate, and the call returns while the gate is closed"""
    import test_stream_contract_gpu as contract
    rig = contract.Rig(eng)
    case_list = []
    for label, name in (("tree_weights", "alternating"), ("tree_weights large", "many-gates")):
        c = next(c for c in tw.cases() if c["label"] == name)
        fn = (lambda h: lambda held: h.weights(held.reshape(-1)))(handles[name])
        case_list.append((label, fn, (np.ascontiguousarray(c["held"][:5]),), None))
    wrong = contract.run_family(rig, "tree weights", case_list)
    assert not wrong, "\n".join(wrong)
    assert "gpbc_fr_tree_weights_dev" in rig.seen


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_lists_in_another_order_share_as_before_and_reconstruct(eng, tensors):
    """a handle is made for a list whose gates' children alternate (parent < child is all a list needs); it shares as the restatement
    does, in list order, and its weights for every held mask are decrypt_plan's"""
    for name, nodes in tw.OTHER_ORDERS.items():
        t = eng.ShareTree(nodes)
        try:
            L, C = t.leaves, t.coeffs
            secrets, coeffs = sc.rand("twg-other-s-" + name, 3), sc.rand("twg-other-q-" + name, 3 * C)
            s, q = fc.rows(secrets).reshape(-1), fc.rows(coeffs).reshape(-1)
            shares = t.share(dev(s) if tensors else s, dev(q) if tensors else q)
            want = [v for j in range(3) for v in tw.list_share(nodes, secrets[j], coeffs[j * C:(j + 1) * C])]
            assert fc.ints(shares.cpu().numpy() if tensors else shares) == want, name
            held = tw.all_masks(L)
            w, ok = t.weights(dev(held.reshape(-1)) if tensors else held.reshape(-1))
            w, ok = (w.cpu().numpy(), ok.cpu().numpy()) if tensors else (w, ok)
            rows = [tw.list_expected(nodes, m) for m in held]
            assert fc.ints(w) == [v for row, _ in rows for v in row] and ok.tolist() == [o for _, o in rows], name
        finally:
            t.close()
