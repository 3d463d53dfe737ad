"""Threshold-tree forests on the device (run with -m gpu): gpbc_fr_share_forest and gpbc_fr_forest_weights, host and _dev forms, on every
case of tests/forest_cases.py against Python integers, byte for byte, into caller buffers with a guard row behind them; a forest of one
tree against ShareTree on that tree at both LDS instances; the weights as device scalars against the shares (fr_mul and a sum give the
secret back); the refusals of a live handle; the stream contract of both _dev entries (the gated procedure of
tests/test_stream_contract_gpu.py) at both LDS instances."""
import numpy as np
import pytest

import fr_cases as fc
import share_cases as sc
import tree_weight_cases as tw
import forest_cases as fo

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
def forests(eng):
    """one handle per forest of the case list"""
    made = {name: eng.ShareForest([fo.tree(l)["nodes"] for l in labels]) for name, labels in fo.FORESTS.items()}
    yield made
    for h in made.values():
        h.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_ids(ids):
    import torch
    return dev(np.ascontiguousarray(ids, dtype=np.uint32).view(np.uint8)).view(torch.int32)


def guarded(forests, entry, tensors):
    """share() or weights() into caller buffers one row longer than the result, filled with a guard byte"""
    import torch

    def call(c):
        k, L = c["k"], c["Lmax"]
        rows, ok = np.full((k * L + 1, 32), GUARD, dtype=np.uint8), np.full(k + 1, GUARD, dtype=np.uint8)
        f = forests[c["forest"]]
        assert (f.trees, f.leaves, f.coeffs, f.tree_leaves, f.tree_coeffs) == (c["T"], L, c["Cmax"], c["L"], c["C"])
        ins = (c["secrets"].reshape(-1), c["coeffs"].reshape(-1)) if entry == "share" else (c["held"].reshape(-1),)
        if tensors:
            rows, ok = dev(rows), dev(ok)
            r, o = getattr(f, entry)(dev_ids(c["tree_of"]), *[dev(a) for a in ins], out=rows[:k * L], ok_out=ok[:k])
            assert r.data_ptr() == rows.data_ptr() and o.data_ptr() == ok.data_ptr()
            torch.cuda.synchronize()
            rows, ok = rows.cpu().numpy(), ok.cpu().numpy()
        else:
            r, o = getattr(f, entry)(c["tree_of"], *ins, out=rows[:k * L], ok_out=ok[:k])
            assert r.ctypes.data == rows.ctypes.data and o.ctypes.data == ok.ctypes.data
        assert (rows[k * L] == GUARD).all() and ok[k] == GUARD, c["label"]
        return rows[:k * L], ok[:k]
    return call


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_share_forest_cases(forests, tensors):
    assert fo.run_share(guarded(forests, "share", tensors), fo.cases()) == []


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_forest_weight_cases(forests, tensors):
    assert fo.run_weights(guarded(forests, "weights", tensors), fo.cases()) == []


@pytest.mark.parametrize("label", ["alternating", "many-gates"])
def test_a_forest_of_one_tree_is_share_tree(eng, label):
    """byte for byte, share and weights, at the small and the large LDS instance"""
    c = next(c for c in tw.cases() if c["label"] == label)
    nodes, k = sc.preorder(c["tree"]), c["k"]
    tree, forest = eng.ShareTree(nodes), eng.ShareForest([nodes])
    try:
        assert (forest.trees, forest.leaves, forest.coeffs) == (1, tree.leaves, tree.coeffs)
        ids = np.zeros(k, dtype=np.uint32)
        secrets, coeffs = fc.rows(sc.rand("fg-one-s-" + label, k)).reshape(-1), fc.rows(sc.rand("fg-one-q-" + label, k * tree.coeffs)).reshape(-1)
        want = tree.share(secrets, coeffs)
        got, ok = forest.share(ids, secrets, coeffs)
        assert want.any() and got.tobytes() == want.tobytes() and ok.all()
        got, ok = forest.share(dev_ids(ids), dev(secrets), dev(coeffs))
        assert got.cpu().numpy().tobytes() == want.tobytes() and ok.cpu().numpy().all()
        held = np.ascontiguousarray(c["held"]).reshape(-1)
        want_w, want_ok = tree.weights(held)
        w, ok = forest.weights(ids, held)
        assert 0 < want_ok.sum() < k and w.tobytes() == want_w.tobytes() and ok.tobytes() == want_ok.tobytes()
        w, ok = forest.weights(dev_ids(ids), dev(held))
        assert w.cpu().numpy().tobytes() == want_w.tobytes() and ok.cpu().numpy().tobytes() == want_ok.tobytes()
    finally:
        tree.close()
        forest.close()


def test_weights_recombine_the_shares_on_the_device(eng, forests):
    """share() and weights() of one forest on the same tree ids, both left on the device: fr_mul of the two and a sum over the Lmax columns
    give every satisfied item's secret back, and 0 for the others"""
    for label in ("mixed/130", "mixed/bad-ids", "edge/65", "large/11"):
        c = next(c for c in fo.cases() if c["label"] == label)
        f, k, L = forests[c["forest"]], c["k"], c["Lmax"]
        ids = dev_ids(c["tree_of"])
        shares, _ = f.share(ids, dev(c["secrets"].reshape(-1)), dev(c["coeffs"].reshape(-1)))
        w, ok = f.weights(ids, dev(c["held"].reshape(-1)))
        prod = eng.fr_mul(w.reshape(-1), shares.reshape(-1)).reshape(k, L, 32)
        acc = prod[:, 0].contiguous()
        for y in range(1, L):
            acc = eng.fr_add(acc.reshape(-1), prod[:, y].contiguous().reshape(-1))
        got, ok = fc.ints(acc.cpu().numpy()), ok.cpu().numpy()
        secrets = fc.ints(c["secrets"])
        assert ok.tolist() == c["want_ok"] and ok.any() and not ok.all(), label
        assert got == [s % R if o else 0 for s, o in zip(secrets, ok)], label


def test_python_values_go_in(eng, forests):
    c = next(c for c in fo.cases() if c["label"] == "mixed/3")
    f = forests["mixed"]
    out, ok = f.share([int(t) for t in c["tree_of"]], fc.ints(c["secrets"]), [fc.ints(row) for row in c["coeffs"]])
    assert fc.ints(out) == c["want_shares"] and ok.tolist() == c["want_valid"] and tuple(out.shape) == (3, c["Lmax"], 32)
    w, ok = f.weights([int(t) for t in c["tree_of"]], [[bool(v) for v in row] for row in c["held"]])
    assert fc.ints(w) == c["want_w"] and ok.tolist() == c["want_ok"]
    with eng.ShareForest([[(sc.ROOT_MARK, 0)], [(sc.ROOT_MARK, 0)]]) as leaves:      # Cmax == 0: no coefficients at all
        out, ok = leaves.share([1, 0, 2], [5, R + 6, 7])
        assert fc.ints(out) == [5, 6, 0] and ok.tolist() == [1, 1, 0]
        w, ok = leaves.weights([0, 1, 2, 0], [[1], [0], [1], [0x80]])
        assert fc.ints(w) == [1, 0, 0, 1] and ok.tolist() == [1, 0, 0, 1]
    with pytest.raises(ValueError, match="closed"):
        leaves.share([0], [1])


def test_a_live_handle_refuses_what_the_header_says(eng, forests):
    """GPBC_ERR_INVALID_ARG before any launch, nothing written: null pointers, overlapping buffers, too many items; k = 0 is a no-op"""
    import torch
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    f = forests["mixed"]                                                              # Lmax 65, Cmax 64: 2 items are 4160 bytes of shares
    h = f._h
    buf = torch.zeros(1 << 15, dtype=torch.uint8, device="cuda")
    hbuf = np.zeros(1 << 15, dtype=np.uint8)
    for share, weights, base, extra in ((lib.gpbc_fr_share_forest, lib.gpbc_fr_forest_weights, hbuf.ctypes.data, []),
                                        (lib.gpbc_fr_share_forest_dev, lib.gpbc_fr_forest_weights_dev, buf.data_ptr(), [None])):
        ids, s, q, out, ok = base, base + 64, base + 128, base + 8192, base + 16384
        bad = [((None, s, q, 2, out, ok), b"null"), ((ids, None, q, 2, out, ok), b"null"), ((ids, s, None, 2, out, ok), b"null"), ((ids, s, q, 2, None, ok), b"null"),
               ((ids, s, q, 1 << 29, out, ok), b"too many items"), ((ids, s, q, (1 << 64) - 1, out, ok), b"too many items"),
               ((ids, s, q, 2, ids + 4, ok), b"overlaps"), ((ids, s, q, 2, s + 32, ok), b"overlaps"), ((ids, s, q, 2, q + 4095, ok), b"overlaps"),
               ((ids, s, q, 2, out, out + 4159), b"overlaps"), ((ids, s, q, 2, out, s + 63), b"overlaps")]
        for args, why in bad:
            assert share(h, *args, *extra) == -1 and why in lib.gpbc_last_error(), (args[3], why, lib.gpbc_last_error())
        assert share(h, None, None, None, 0, None, None, *extra) == 0
        held, w = base + 64, base + 8192
        bad = [((None, held, 2, w, ok), b"null"), ((ids, None, 2, w, ok), b"null"), ((ids, held, 2, None, ok), b"null"), ((ids, held, 2, w, None), b"null"),
               ((ids, held, 1 << 29, w, ok), b"too many items"), ((ids, held, 2, held + 129, ok), b"overlaps"), ((ids, held, 2, w, ids + 7), b"overlaps"),
               ((ids, held, 2, w, w + 4159), b"overlaps")]
        for args, why in bad:
            assert weights(h, *args, *extra) == -1 and why in lib.gpbc_last_error(), (args[2], why, lib.gpbc_last_error())
        assert weights(h, None, None, 0, None, None, *extra) == 0
    torch.cuda.synchronize()
    assert not buf.any().item() and not hbuf.any()
    assert lib.gpbc_share_forest_tree_leaves(h, 5) == 0 and lib.gpbc_share_forest_tree_coeffs(h, 1 << 40) == 0 and lib.gpbc_share_forest_tree_leaves(h, 4) == 65
    with pytest.raises(ValueError, match="overlaps"):
        f.weights(buf[:8].view(torch.int32), buf[8:8 + 130], out=buf[:2 * 65 * 32])
    assert tuple(f.weights(buf[:0].view(torch.int32), buf[:0])[0].shape) == (0, 65, 32)


def test_dev_forms_are_ordered_on_the_callers_stream_and_do_not_wait(eng, forests):
    """the gated procedure of tests/test_stream_contract_gpu.py on both entries at both LDS instances: the results are those of the real
    inputs copied in behind a closed gate, and the calls return while the gate is closed.  Tree ids travel as [k, 4] bytes there."""
    import torch
    import test_stream_contract_gpu as contract
    rig = contract.Rig(eng)
    as_ids = lambda b: b.reshape(-1).view(torch.int32) if torch.is_tensor(b) else np.ascontiguousarray(b).reshape(-1).view(np.uint32)
    case_list = []
    for label, name in (("small", "mixed/65"), ("large", "large/11")):
        c = next(c for c in fo.cases() if c["label"] == name)
        f, k = forests[c["forest"]], 5
        ids8 = np.ascontiguousarray(c["tree_of"][:k]).view(np.uint8).reshape(k, 4)
        share = (lambda f: lambda ids, s, q: f.share(as_ids(ids), s.reshape(-1), q.reshape(-1)))(f)
        weights = (lambda f: lambda ids, held: f.weights(as_ids(ids), held.reshape(-1)))(f)
        case_list.append(("share_forest " + label, share, (ids8, c["secrets"][:k], np.ascontiguousarray(c["coeffs"][:k]).reshape(k, -1)), None))
        case_list.append(("forest_weights " + label, weights, (ids8, np.ascontiguousarray(c["held"][:k])), None))
    wrong = contract.run_family(rig, "forests", case_list)
    assert not wrong, "\n".join(wrong)
    assert {"gpbc_fr_share_forest_dev", "gpbc_fr_forest_weights_dev"} <= rig.seen
