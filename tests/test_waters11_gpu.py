"""Waters11 CP-ABE batched decryption on the MI355X (run with -m gpu): waters11.decrypt_batch on the engine.

  * four ciphertexts under four different policies in one batch (AND / OR, 3 of 5, one row padded up, one the key does not satisfy),
    host arrays and CUDA tensors: ok = [1, 1, 1, 0], a zero row, the other messages byte-identical to the plaintexts and to the
    scheme's row-by-row Decrypt on the oracle;
  * 2^12 ciphertexts of 16 rows cycling through four policy shapes, every 64th unsatisfied, everything in HBM: ok exact, every
    decryptable message equal to its plaintext, the rest zero rows, the first 256 rows of weights equal to the Python elimination,
    four ciphertexts equal to the oracle Decrypt;
  * the device-weights and the host-weights routes agree on 64 ciphertexts."""
import numpy as np
import pytest

import fr_cases as fc
from waters11_fixture import Instance, at_size_policies, small_policies
from gopairingbasedcryptography_amd import lw11, waters11

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


@pytest.mark.parametrize("on_device", [False, True])
def test_four_policies_in_one_batch(eng, oracle, on_device):
    import torch
    pols, key = small_policies()
    inst = Instance(eng, key, pols, dev=torch.device("cuda") if on_device else None, tag="gpu4")
    out, ok = waters11.decrypt_batch(eng, inst.key, pols, inst.c, inst.c_prime, inst.cx, inst.dx)
    assert _is_cuda(out) == on_device and _is_cuda(ok) == on_device
    out, ok, msgs = inst.host(out), inst.host(ok), inst.host(inst.msgs).reshape(-1, 384)
    assert out.shape == (4, 384) and ok.tolist() == [1, 1, 1, 0] and not out[3].any()
    for t in range(3):
        assert (out[t] == msgs[t]).all(), t
        assert (out[t] == inst.row_by_row_decrypt(oracle, t)).all(), t


def _is_cuda(a):
    return type(a).__module__.startswith("torch") and a.is_cuda


@pytest.fixture(scope="module")
def at_size(eng):
    import torch
    n = 1 << 12
    pols, key = at_size_policies(n)
    return Instance(eng, key, pols, rows=16, dev=torch.device("cuda"), tag="size"), pols, key


def test_at_size(eng, oracle, at_size):
    import torch
    inst, pols, key = at_size
    n = len(pols)
    pad = waters11.pad_policies(pols, rows=16)
    assert (pad.rows, pad.cols) == (16, 16)
    out, ok = waters11.decrypt_batch(eng, inst.key, pad, inst.c, inst.c_prime, inst.cx, inst.dx)
    torch.cuda.synchronize()
    want_ok = np.array([0 if j % 64 == 63 else 1 for j in range(n)], dtype=np.uint8)
    assert inst.satisfied()[:130] == want_ok[:130].astype(bool).tolist()
    ok, out, msgs = ok.cpu().numpy(), out.cpu().numpy(), inst.msgs.reshape(n, 384).cpu().numpy()
    assert (ok == want_ok).all()
    assert (out[want_ok == 1] == msgs[want_ok == 1]).all() and not out[want_ok == 0].any()
    held = waters11.held_mask(pad.rho, key)
    w, wok = eng.fr_lsss_weights(torch.from_numpy(pad.matrix[:256]).cuda().reshape(-1), 16, 16, torch.from_numpy(held[:256]).cuda().reshape(-1))
    w = np.asarray(fc.ints(w.cpu().numpy()), dtype=object).reshape(256, 16)
    for j in range(256):
        m, rho = pols[j]
        got = lw11.reconstruction_weights(m, rho, key)
        exp = [0] * 16
        if got is not None:
            for x, wx in zip(*got):
                exp[x] = wx
        assert w[j].tolist() == exp and int(wok[j]) == (got is not None), j
    for j in (0, 1, 2, 3):
        assert (out[j] == inst.row_by_row_decrypt(oracle, j)).all(), j


def test_device_and_host_weight_routes_agree(eng, at_size):
    inst, pols, key = at_size
    n = 64
    part = lambda a, width: a.reshape(-1, width)[:n * (a.numel() // width // len(pols))].contiguous()
    args = (part(inst.c, 384), part(inst.c_prime, 128), part(inst.cx, 64), part(inst.dx, 128))
    out_d, ok_d = waters11.decrypt_batch(eng, inst.key, waters11.pad_policies(pols[:n], rows=16), *args)
    out_h, ok_h = waters11.decrypt_batch_host_weights(eng, inst.key, [(m, rho) for m, rho in pols[:n]], *args)
    assert ok_d.cpu().tolist() == ok_h.cpu().tolist() == [1] * 63 + [0]
    assert bool((out_d == out_h).all())
