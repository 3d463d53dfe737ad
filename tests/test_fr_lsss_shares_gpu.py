"""LSSS share generation on the device (run with -m gpu): gpbc_fr_lsss_shares, host and _dev forms, one matrix for all vectors and a
matrix per vector, on the shapes of tests/indexed_cases.py against Python integers, exactly; outputs canonical; and the shares recombine
under the weights of the existing fr_lsss_weights to the secret."""
import pytest

import indexed_cases as ic
from lw11_fixture import and_chain_policy, threshold_policy

pytestmark = pytest.mark.gpu
R, K = ic.R, 67


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("per_item", [False, True], ids=["shared", "per-item"])
@pytest.mark.parametrize("rows,cols", ic.SHARE_SHAPES)
def test_shares_against_python_integers(eng, rows, cols, per_item, tensors):
    import torch
    case = ic.shares_case(rows, cols, K, per_item)
    m, v = ic.matrix_rows(case), ic.vector_rows(case)
    if tensors:
        side = torch.cuda.Stream()
        md, vd = torch.from_numpy(m).cuda(), torch.from_numpy(v).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            out = eng.fr_lsss_shares(md, vd, rows, cols)
        side.synchronize()
        assert out.is_cuda
        out = out.cpu().numpy()
    else:
        out = eng.fr_lsss_shares(m, v, rows, cols)
    assert out.shape == (K, rows, 32) and ic.ints(out) == [x for r in case["want"] for x in r]


def test_python_integers_one_vector_and_out(eng):
    import torch
    case = ic.shares_case(4, 3, 1, False)
    assert eng.fr_to_ints(eng.fr_lsss_shares(case["matrix"][0], case["vectors"])) == case["want"][0]
    case = ic.shares_case(16, 15, 5, True)
    out = torch.zeros((5, 16, 32), dtype=torch.uint8, device="cuda")
    got = eng.fr_lsss_shares(torch.from_numpy(ic.matrix_rows(case)).cuda(), torch.from_numpy(ic.vector_rows(case)).cuda(), 16, 15, out=out)
    assert got is out and ic.ints(out.cpu().numpy()) == [x for r in case["want"] for x in r]
    buf = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        eng.fr_lsss_shares(buf[:12 * 32], buf[12 * 32:15 * 32], 4, 3, out=buf[14 * 32:18 * 32])


@pytest.mark.parametrize("policy,held", [(and_chain_policy(16), list(range(16))), (threshold_policy(8, 16), [1, 2, 4, 7, 8, 11, 13, 15]), (threshold_policy(3, 5), [0, 2, 3])],
                         ids=["and-chain-16", "8-of-16", "3-of-5"])
def test_shares_recombine_under_the_lsss_weights(eng, policy, held):
    """sum_x w_x lambda_x = s for the weights fr_lsss_weights gives on a satisfying held set"""
    matrix, _ = policy
    rows, cols = len(matrix), len(matrix[0])
    m = [[v % R for v in row] for row in matrix]
    vectors = [[ic.o.bench_scalar("lsss-recombine-%d" % c, j) for c in range(cols)] for j in range(K)]
    lam = eng.fr_to_ints(eng.fr_lsss_shares(m, vectors))
    mask = [[1 if x in held else 0 for x in range(rows)]]
    w, ok = eng.fr_lsss_weights(m, held=mask)
    w = eng.fr_to_ints(w)
    assert ok.tolist() == [1]
    for j in range(K):
        assert sum(w[x] * lam[j * rows + x] for x in range(rows)) % R == vectors[j][0], j
