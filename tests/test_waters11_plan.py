"""Waters11 CP-ABE batched decryption through the host planner gopairingbasedcryptography_amd/waters11.py, on the oracle engine (the
same flow runs on the GPU engine in test_waters11_gpu.py): pad_policies / held_mask / key_index on ragged policies, then a small
instance made by waters11_fixture.py from known secrets — four ciphertexts under four different policies in one batch return the
messages, byte-identical to the scheme's row-by-row Decrypt written out with oracle calls, the unsatisfied one gives ok = 0 and a
zero row; the host-weights route gives the same."""
import numpy as np
import pytest

import bn254_py as o
from standin_engine import StandInEngine, TensorEngine, same_on_tensors, tensors
from waters11_fixture import Instance, and_or_16, small_policies
from gopairingbasedcryptography_amd import lw11, waters11

R = o.R


def test_pad_policies_and_masks():
    pols, key = small_policies()
    pad = waters11.pad_policies(pols)
    assert pad.matrix.shape == (4, 5, 3, 32) and pad.rho.shape == (4, 5) and (pad.rows, pad.cols) == (5, 3)
    ints = lambda a: [int.from_bytes(r.tobytes(), "little") for r in a.reshape(-1, 32)]
    assert ints(pad.matrix[0]) == [1, 1, 0, 0, R - 1, 0, 1, 0, 1, 0, 0, R - 1, 0, 0, 0]       # -1 as r - 1, a padded row of zeros
    assert ints(pad.matrix[2]) == [1] + [0] * 14                                                # padded rows and columns
    assert pad.rho[0].tolist() == [11, 22, 33, 44, -1] and pad.rho[2].tolist() == [500, -1, -1, -1, -1]
    held = waters11.held_mask(pad.rho, key)
    assert held.dtype == np.uint8 and held.tolist() == [[1, 1, 0, 0, 0], [0, 1, 0, 1, 1], [1, 0, 0, 0, 0], [1, 0, 1, 0, 0]]
    idx = waters11.key_index(pad.rho, key)
    skey = sorted(key)
    assert all(skey[idx[t, x]] == pad.rho[t, x] for t in range(4) for x in range(5) if held[t, x]) and (idx[held == 0] == len(key)).all()
    assert waters11.held_mask(pad.rho, []).sum() == 0
    wide = waters11.pad_policies(pols, rows=8, cols=4)
    assert wide.matrix.shape == (4, 8, 4, 32) and (wide.matrix[:, :5, :3] == pad.matrix).all() and not wide.matrix[:, 5:].any() and not wide.matrix[:, :, 3:].any()
    for bad in (lambda: waters11.pad_policies(pols, rows=4), lambda: waters11.pad_policies([([[1, 2], [3]], [1, 2])]), lambda: waters11.pad_policies([([[1]], [-5])]),
                lambda: waters11.pad_policies([([[1]], [1, 2])]), lambda: waters11.held_mask(pad.rho, [3, 3])):
        with pytest.raises(ValueError):
            bad()


def test_and_or_16_is_what_it_says():
    m, rho = and_or_16()
    assert len(m) == 16 and all(len(r) == 15 for r in m)
    assert lw11.reconstruction_weights(m, rho, rho[:8]) == (list(range(8)), [1] * 8)
    assert lw11.reconstruction_weights(m, rho, rho[8:]) == (list(range(8, 16)), [1] * 8)
    assert lw11.reconstruction_weights(m, rho, rho[1:15]) is None


def test_decrypt_matches_the_row_by_row_decrypt(oracle):
    eng = StandInEngine(oracle)
    pols, key = small_policies()
    inst = Instance(eng, key, pols, tag="plan")
    assert inst.satisfied() == [True, True, True, False]
    calls = []
    eng.multi_pair = lambda P, Q, off, f=eng.multi_pair: calls.append(("multi_pair", len(off) - 1, np.asarray(P).size // 64)) or f(P, Q, off)
    eng.gt_exp = lambda *a: pytest.fail("no GT exponentiation in the planner")
    out, ok = waters11.decrypt_batch(eng, inst.key, pols, inst.c, inst.c_prime, inst.cx, inst.dx)
    assert calls == [("multi_pair", 4, 4 * (5 + 2))]
    assert out.shape == (4, 384) and ok.tolist() == [1, 1, 1, 0] and not out[3].any()
    out_h, ok_h = waters11.decrypt_batch_host_weights(eng, inst.key, pols, inst.c, inst.c_prime, inst.cx, inst.dx)
    out_p, ok_p = waters11.decrypt_batch(eng, inst.key, waters11.pad_policies(pols), inst.c, inst.c_prime, inst.cx, inst.dx)
    assert (out_h == out).all() and ok_h.tolist() == ok.tolist() and (out_p == out).all() and ok_p.tolist() == ok.tolist()
    del eng.gt_exp
    # the planner's tensor path, on CPU tensors: tensors with the same bytes and the same ok rows
    out_t, ok_t = waters11.decrypt_batch(TensorEngine(eng), inst.key, pols, *tensors(inst.c, inst.c_prime, inst.cx, inst.dx))
    assert same_on_tensors(out_t, np.asarray(out)) and same_on_tensors(ok_t, np.asarray(ok))
    for t in range(3):
        assert (out[t] == np.asarray(inst.msgs)[t]).all(), t
        assert (out[t] == inst.row_by_row_decrypt(oracle, t)).all(), t
    assert inst.row_by_row_decrypt(oracle, 3) is None


def test_decrypt_argument_checks(oracle):
    eng = StandInEngine(oracle)
    pols, key = small_policies()
    inst = Instance(eng, key, pols[:2], tag="args")
    with pytest.raises(ValueError):
        waters11.decrypt_batch(eng, inst.key, pols[:2], inst.c, inst.c_prime, np.asarray(inst.cx)[:-1], inst.dx)
    with pytest.raises(ValueError):
        waters11.decrypt_batch(eng, inst.key, pols[:1], inst.c, inst.c_prime, inst.cx, inst.dx)
    eng.multi_pair = eng.g1_scalar_mul = eng.fr_lsss_weights = lambda *a: pytest.fail("no engine call without a ciphertext")
    z = np.zeros(0, dtype=np.uint8)
    out, ok = waters11.decrypt_batch(eng, inst.key, [], z, z, z, z)
    assert out.shape == (0, 384) and ok.shape == (0,)
