"""LW11 decentralised ABE batched decryption on the MI355X (run with -m gpu) through gopairingbasedcryptography_amd/lw11.py: the
small instances of test_lw11_plan.py on the GPU engine (host arrays and CUDA tensors), then at size — 2^14 ciphertexts under one
16-row policy (16 of 16 Shamir rows: Lagrange weights, none 0 or 1) and 2^12 under one 64-row policy (an AND chain: all weights 1).
The instances are made by tests/lw11_fixture.py from known secrets with the engine's OTHER entries (pair_batch, gt_exp, the
shared-base scalar multiplications); every message is recovered byte for byte, and 4 ciphertexts of each are also decrypted row by
row in the reference's shape with oracle calls."""
import numpy as np
import pytest

from lw11_fixture import Instance, and_chain_policy, and_or_policy, threshold_policy
from gopairingbasedcryptography_amd import lw11

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda", 0)


def test_small_instances_host_and_device(eng, oracle, dev):
    import torch
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for (m, rho), attrs, unit in ((and_or_policy(), [11, 22, 44], True), (threshold_policy(3, 4), [200, 201, 203], False)):
        inst = Instance(eng, m, rho, attrs, n_ct=3)
        rows, w = lw11.reconstruction_weights(m, rho, inst.user_attrs)
        folded = lw11.fold_key(eng, rows, w, inst.h_gid, inst.k_by_row)
        out = lw11.decrypt_batch(eng, folded, inst.c0, inst.c1, inst.c2, inst.c3)
        assert (out == inst.msgs).all()
        out_d = lw11.decrypt_batch(eng, folded, put(inst.c0), put(inst.c1), put(inst.c2), put(inst.c3))
        assert (out_d.cpu().numpy() == out).all()
        for t in range(3):
            assert (out[t] == inst.row_by_row_decrypt(oracle, t, rows, w, running=unit)).all()


@pytest.mark.parametrize("shape", ["2^14 x 16 rows", "2^12 x 64 rows"])
def test_decrypt_at_size(eng, oracle, dev, shape):
    import torch
    if shape == "2^14 x 16 rows":
        n, (m, rho), unit = 1 << 14, threshold_policy(16, 16), False
    else:
        n, (m, rho), unit = 1 << 12, and_chain_policy(64), True
    inst = Instance(eng, m, rho, rho, n_ct=n, dev=dev, tag=shape[:4])
    rows, w = lw11.reconstruction_weights(m, rho, inst.user_attrs)
    assert rows == list(range(len(rho))) and (all(x == 1 for x in w) if unit else all(x not in (0, 1) for x in w))
    folded = lw11.fold_key(eng, rows, w, inst.h_gid, inst.k_by_row)
    out = lw11.decrypt_batch(eng, folded, inst.c0, inst.c1, inst.c2, inst.c3)
    torch.cuda.synchronize()
    wrong = torch.nonzero((out != inst.msgs).any(dim=1)).flatten()
    print("%s: %d of %d messages differ" % (shape, wrong.numel(), n))
    assert out.shape == (n, 384) and wrong.numel() == 0, wrong[:8].tolist()
    assert not bool((inst.msgs[0] == inst.msgs[1]).all())
    for t in (0, 1, n // 2, n - 1):
        assert (inst.row_by_row_decrypt(oracle, t, rows, w, running=unit) == out[t].cpu().numpy()).all(), t
    # a key that lacks one attribute of an all-rows policy cannot be folded
    assert lw11.reconstruction_weights(m, rho, set(rho) - {rho[3]}) is None
