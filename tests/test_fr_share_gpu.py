"""Secret sharing in Fr on the device (run with -m gpu): gpbc_fr_poly_eval and gpbc_fr_share_tree, host and _dev forms, numpy and
tensors, on every case of tests/share_cases.py against its Python-integer restatement, byte for byte; canonical outputs; the stream
contract of the two _dev entries (the gated procedure of tests/test_stream_contract_gpu.py); one handle over several calls."""
import numpy as np
import pytest

import fr_cases as fc
import share_cases as sc

pytestmark = pytest.mark.gpu
R = fc.R


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(a):
    return a.cpu().numpy() if not isinstance(a, np.ndarray) else a


def direct(eng, tensors, c, nc, d, p, npts, m, k):
    import torch
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    if not tensors:
        out = np.zeros((k, m, 32), dtype=np.uint8)
        _lib.check(lib.gpbc_fr_poly_eval(c.ctypes.data, nc, d, p.ctypes.data, npts, m, k, out.ctypes.data))
        return out
    cd, pd, out = dev(c), dev(p), torch.zeros((k, m, 32), dtype=torch.uint8, device="cuda")
    _lib.check(lib.gpbc_fr_poly_eval_dev(cd.data_ptr(), nc, d, pd.data_ptr(), npts, m, k, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return host(out)


def poly_call(eng, tensors):
    def call(c, nc, d, p, npts, m, k):
        if max(nc, npts) != k:                                                      # one row of each for k rows: the wrapper has no k, the C entries do
            return direct(eng, tensors, c, nc, d, p, npts, m, k)
        out = eng.fr_poly_eval(dev(c) if tensors else c, dev(p) if tensors else p, d, m)
        assert tuple(out.shape) == (k, m, 32)
        return host(out)
    return call


def tree_call(eng, tensors, trees=None):
    def call(nodes, secrets, coeffs, k):
        t = eng.ShareTree(nodes)
        try:
            out = t.share(dev(secrets) if tensors else secrets, dev(coeffs) if tensors else coeffs)
            assert tuple(out.shape) == (k, t.leaves, 32)
            return host(out)
        finally:
            t.close()
    return call


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_poly_eval_cases(eng, tensors):
    assert sc.run_poly_cases(poly_call(eng, tensors), sc.poly_cases() + [sc.poly_big_case()]) == []


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_tree_cases(eng, tensors):
    assert sc.run_tree_cases(tree_call(eng, tensors), sc.tree_cases()) == []


def test_python_integers_go_in(eng):
    c = sc.poly_row_cases()[3]
    assert eng.fr_to_ints(eng.fr_poly_eval(c["coeffs"], c["points"])) == sc.poly_expected(c)
    t = next(c for c in sc.tree_cases() if c["label"] == "alternating")
    tree = eng.ShareTree(sc.preorder(t["tree"]))
    assert (tree.leaves, tree.coeffs) == (len(sc.tree_expected(t)) // t["k"], sc.n_coeffs(t["tree"]))
    assert eng.fr_to_ints(tree.share(t["secrets"], t["coeffs"])) == sc.tree_expected(t)
    tree.close()
    with pytest.raises(ValueError):
        tree.share(t["secrets"], t["coeffs"])                                        # closed


def test_outputs_are_canonical(eng):
    """fr_add(., 0) reduces its operand: a canonical output comes back unchanged"""
    zero = fc.rows([0]).reshape(-1)
    for c in sc.poly_value_cases():
        out = eng.fr_poly_eval(c["coeffs"], c["points"]).reshape(-1)
        assert (eng.fr_add(out, zero).reshape(-1) == out).all() and max(fc.ints(out)) < R, c["label"]
    for label in ("leaf", "1-of-5", "3-of-3", "example"):
        c = next(c for c in sc.tree_cases() if c["label"] == label)
        tree = eng.ShareTree(sc.preorder(c["tree"]))
        out = tree.share(c["secrets"], c["coeffs"]).reshape(-1)
        tree.close()
        assert (eng.fr_add(out, zero).reshape(-1) == out).all() and max(fc.ints(out)) < R, label


def test_out_argument_and_overlap(eng):
    import torch
    c = sc.poly_row_cases()[3]
    cb, pb = sc.rows([v for r in c["coeffs"] for v in r]), sc.rows([v for r in c["points"] for v in r])
    out = torch.zeros((c["k"], c["m"], 32), dtype=torch.uint8, device="cuda")
    assert eng.fr_poly_eval(dev(cb), dev(pb), c["d"], c["m"], out=out) is out and fc.ints(host(out)) == sc.poly_expected(c)
    buf = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        eng.fr_poly_eval(buf[:5 * 32], buf[32:8 * 32], 5, 7, out=buf[2 * 32:9 * 32])
    tree = eng.ShareTree(sc.preorder(sc.flat_gate(2, 3)))
    with pytest.raises(ValueError):
        tree.share(buf[:2 * 32], buf[2 * 32:4 * 32], out=buf[32:7 * 32])
    with pytest.raises(ValueError):
        tree.share(buf[:2 * 32], buf[2 * 32:5 * 32])                                 # three coefficients for two items of one
    with pytest.raises(ValueError):
        tree.share(buf[:2 * 32], None)
    assert tuple(tree.share(buf[:0], buf[:0]).shape) == (0, 3, 32)                   # no items: a no-op
    tree.close()
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    assert lib.gpbc_fr_poly_eval_dev(buf.data_ptr(), 1, 4, buf.data_ptr() + 4 * 32, 1, 4, 2, buf.data_ptr() + 6 * 32, None) == -1 and b"overlaps" in lib.gpbc_last_error()


def test_one_handle_many_calls_and_after_release(eng):
    c = next(c for c in sc.tree_cases() if c["label"] == "example")
    want = sc.tree_expected(c)
    tree = eng.ShareTree(sc.preorder(c["tree"]))
    s, q = sc.rows(c["secrets"]), sc.rows([v for r in c["coeffs"] for v in r])
    for _ in range(3):
        assert fc.ints(tree.share(s, q)) == want and fc.ints(host(tree.share(dev(s), dev(q)))) == want
    eng.release_workspaces()
    assert fc.ints(tree.share(s, q)) == want and fc.ints(host(tree.share(dev(s), dev(q)))) == want
    L = tree.leaves
    assert fc.ints(tree.share(s[:32], q[:tree.coeffs * 32])) == want[:L]             # another item count on the same handle
    tree.close()
    tree.close()


def test_dev_forms_are_ordered_on_the_callers_stream_and_do_not_wait(eng):
    """the gated procedure of tests/test_stream_contract_gpu.py on both _dev entries, each at both of its LDS instances: the results are
    those of the real inputs copied in behind a closed gate, and the call returns while the gate is closed"""
    import test_stream_contract_gpu as contract
    rig = contract.Rig(eng)
    rows2 = lambda v: fc.rows(v)
    small, long_ = sc._poly("gate-small", 16, 24, 5), sc._poly("gate-long", 300, 2, 5)
    trees = {"fr_share_tree": sc.alternating(), "fr_share_tree large": sc.flat_gate(330, 330)}
    handles = {name: eng.ShareTree(sc.preorder(t)) for name, t in trees.items()}
    case_list = []
    for label, c in (("fr_poly_eval", small), ("fr_poly_eval long", long_)):
        fn = (lambda d, m: lambda cb, pb: eng.fr_poly_eval(cb.reshape(-1), pb.reshape(-1), d, m))(c["d"], c["m"])
        case_list.append((label, fn, (rows2([v for r in c["coeffs"] for v in r]), rows2([v for r in c["points"] for v in r])), None))
    for label, h in handles.items():
        k = 5
        fn = (lambda h: lambda s, q: h.share(s.reshape(-1), q.reshape(-1)))(h)
        case_list.append((label, fn, (rows2(sc.rand("gate-s-" + label, k)), rows2(sc.rand("gate-q-" + label, k * h.coeffs))), None))
    try:
        wrong = contract.run_family(rig, "share", case_list)
    finally:
        for h in handles.values():
            h.close()
    assert not wrong, "\n".join(wrong)
    assert {"gpbc_fr_poly_eval_dev", "gpbc_fr_share_tree_dev"} <= rig.seen
