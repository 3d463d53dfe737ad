"""Waters11 CP-ABE from boolean formulas on the device (run with -m gpu): 24 ciphertexts, each under a formula of its own with 1 to 8
leaves — attributes repeat, and the key does not satisfy every formula — encrypted by waters11.encrypt_batch on formula.padded(...), whose
matrix is built by gpbc_fr_lsss_from_formula, then decrypted by decrypt_batch_formulas (the 0 / 1 route: formula_select, sums and one
negation) and by decrypt_batch (the field solve): messages and ok are byte-identical, the satisfied items return the plaintext and the
others zero rows.  On host arrays and on CUDA tensors."""
import numpy as np
import pytest

import bn254_py as o
import formula_cases as fc

pytestmark = pytest.mark.gpu
R = o.R
N_ITEMS, UNIVERSE, KEY = 24, list(range(40, 52)), [40, 41, 43, 44, 46, 47, 50]


def sc(tag, i=0):
    return o.bench_scalar("w11f-" + tag, i)


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def formulas():
    rng = np.random.default_rng(11)
    out = []
    for j in range(N_ITEMS):
        tree = fc.random_tree(1 + j % 8, rng, attrs=len(UNIVERSE))
        relabel = lambda t: UNIVERSE[t] if fc.is_leaf(t) else (t[0], relabel(t[1]), relabel(t[2]))
        out.append(relabel(tree))
    return out


@pytest.fixture(scope="module")
def world(eng):
    from gopairingbasedcryptography_amd import formula
    trees = formulas()
    g1, g2 = eng.generators()
    e = np.asarray(eng.pair_batch(g1, g2)).reshape(1, 384)
    alpha, a, t = sc("alpha"), sc("a"), sc("t")
    tau = {u: sc("tau", u) for u in UNIVERSE}
    g1a = np.asarray(eng.g1_scalar_mul_base([a])).reshape(64)
    e_alpha = np.asarray(eng.gt_exp(e, [alpha])).reshape(384)
    hs = np.asarray(eng.g1_scalar_mul_base([tau[u] for u in UNIVERSE])).reshape(-1, 64)
    kl = np.asarray(eng.g1_scalar_mul_base([(alpha + a * t) % R] + [tau[u] * t % R for u in KEY])).reshape(-1, 64)
    key = (kl[0].copy(), np.asarray(eng.g2_scalar_mul_base([t])).reshape(128), {u: kl[1 + i].copy() for i, u in enumerate(KEY)})
    msgs = np.asarray(eng.gt_exp(np.tile(e, (N_ITEMS, 1)), [sc("msg", j) for j in range(N_ITEMS)])).reshape(N_ITEMS, 384)
    nodes = formula.encode(trees)
    rows, cols = formula.size(nodes)
    rand = lambda tag, shape: eng.fr_to_bytes([sc(tag, i) for i in range(int(np.prod(shape)))]).reshape(*shape, 32).copy()
    sat = [fc.choose(tr, [u in KEY for u in fc.matrix_of(tr)[1]])[0] for tr in trees]
    return dict(trees=trees, nodes=nodes, rows=rows, cols=cols, g1a=g1a, e_alpha=e_alpha, h={u: hs[i] for i, u in enumerate(UNIVERSE)}, key=key, msgs=msgs,
                s=rand("s", (N_ITEMS,)), v=rand("v", (N_ITEMS, cols - 1)), r=rand("r", (N_ITEMS, rows)), sat=sat)


def test_the_batch_is_what_it_claims(world):
    w = world
    assert len(w["trees"]) == 24 and sorted({fc.n_leaves(t) for t in w["trees"]}) == list(range(1, 9)) and w["rows"] == 8
    assert 4 <= sum(w["sat"]) <= 20                                                # both verdicts occur
    rhos = [fc.matrix_of(t)[1] for t in w["trees"]]
    assert any(len(set(r)) < len(r) for r in rhos)                                 # an attribute on more than one leaf
    assert any(s and len(set(r)) < len(r) for s, r in zip(w["sat"], rhos))


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_formula_route_is_the_field_route_byte_for_byte(eng, world, tensors):
    import torch
    from gopairingbasedcryptography_amd import formula, waters11
    w = world
    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if tensors else (lambda a: a)
    host = (lambda a: a.cpu().numpy()) if tensors else np.asarray
    msgs = put(w["msgs"])
    pad = formula.padded(eng, w["nodes"], like=msgs)
    assert (torch.is_tensor(pad.matrix) and pad.matrix.is_cuda) if tensors else isinstance(pad.matrix, np.ndarray)
    want = waters11.pad_policies([fc.matrix_of(t) for t in w["trees"]])
    assert host(pad.matrix).tobytes() == want.matrix.tobytes() and pad.rho.tolist() == want.rho.tolist() and (pad.rows, pad.cols) == (want.rows, want.cols)
    ct = waters11.encrypt_batch(eng, w["g1a"], w["e_alpha"], w["h"], pad, msgs, put(w["s"]), put(w["v"]), put(w["r"]))
    by_formula, ok = waters11.decrypt_batch_formulas(eng, w["key"], put(w["nodes"]) if tensors else w["nodes"], *ct)
    by_solve, ok_solve = waters11.decrypt_batch(eng, w["key"], pad, *ct)
    by_formula, ok, by_solve, ok_solve = host(by_formula), host(ok), host(by_solve), host(ok_solve)
    assert ok.tolist() == ok_solve.tolist() == [int(s) for s in w["sat"]]
    assert by_formula.tobytes() == by_solve.tobytes()
    for j, s in enumerate(w["sat"]):
        assert by_formula[j].tobytes() == (w["msgs"][j].tobytes() if s else bytes(384)), j
