"""The planners' opt-in routes over the segmented multi-scalar multiplication on the MI355X (run with -m gpu), 256 ciphertexts of 16
rows each, everything in HBM: waters11.decrypt_batch(msm=True) against msm=False (messages and ok equal byte for byte, decryptable
messages equal to the plaintexts, every 64th ciphertext unsatisfied and a zero row), and lw11.decrypt_batch_msm against
decrypt_batch (16 of 16 Shamir rows: Lagrange weights, none 0 or 1)."""
import numpy as np
import pytest

from lw11_fixture import Instance as Lw11Instance, threshold_policy
from waters11_fixture import Instance as W11Instance, at_size_policies
from gopairingbasedcryptography_amd import lw11, waters11

pytestmark = pytest.mark.gpu
N, ROWS = 256, 16


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def test_waters11_msm_route(eng):
    import torch
    pols, key = at_size_policies(N)
    inst = W11Instance(eng, key, pols, rows=ROWS, dev=torch.device("cuda"), tag="msm")
    pad = waters11.pad_policies(pols, rows=ROWS)
    out0, ok0 = waters11.decrypt_batch(eng, inst.key, pad, inst.c, inst.c_prime, inst.cx, inst.dx)
    out1, ok1 = waters11.decrypt_batch(eng, inst.key, pad, inst.c, inst.c_prime, inst.cx, inst.dx, msm=True)
    torch.cuda.synchronize()
    assert out1.is_cuda and ok1.is_cuda and out1.shape == (N, 384)
    assert bool((out1 == out0).all()) and bool((ok1 == ok0).all())
    want_ok = np.array([0 if j % 64 == 63 else 1 for j in range(N)], dtype=np.uint8)
    ok, out, msgs = ok1.cpu().numpy(), out1.cpu().numpy(), inst.msgs.reshape(N, 384).cpu().numpy()
    assert (ok == want_ok).all()
    assert (out[want_ok == 1] == msgs[want_ok == 1]).all() and not out[want_ok == 0].any()


def test_lw11_msm_route(eng):
    import torch
    m, rho = threshold_policy(ROWS, ROWS)
    inst = Lw11Instance(eng, m, rho, rho, n_ct=N, dev=torch.device("cuda", 0), tag="msm")
    rows, w = lw11.reconstruction_weights(m, rho, inst.user_attrs)
    assert rows == list(range(ROWS)) and all(x not in (0, 1) for x in w)
    folded = lw11.fold_key(eng, rows, w, inst.h_gid, inst.k_by_row)
    want = lw11.decrypt_batch(eng, folded, inst.c0, inst.c1, inst.c2, inst.c3)
    got = lw11.decrypt_batch_msm(eng, folded, inst.h_gid, inst.c0, inst.c1, inst.c2, inst.c3)
    torch.cuda.synchronize()
    assert got.is_cuda and got.shape == (N, 384)
    assert bool((got == want).all()) and bool((got == inst.msgs).all())
    assert not bool((inst.msgs[0] == inst.msgs[1]).all())
    # host arrays in, host array out, the same bytes
    host = lambda a: a[:4 * (a.numel() // N)].cpu().numpy()
    h = lw11.decrypt_batch_msm(eng, folded, inst.h_gid, host(inst.c0.reshape(-1)), host(inst.c1.reshape(-1)), host(inst.c2.reshape(-1)), host(inst.c3.reshape(-1)))
    assert isinstance(h, np.ndarray) and (h == got[:4].cpu().numpy()).all()
