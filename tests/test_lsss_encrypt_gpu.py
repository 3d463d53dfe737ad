"""Waters11 Encrypt / KeyGenerate, LW11 Encrypt and BSW07 Encrypt with tables on the MI355X (run with -m gpu) through the host planners
on the GPU engine, host arrays and CUDA tensors: the outputs are the fixtures' ciphertext bytes, tables=True is tables=False, and the
existing decryptors recover every message of a satisfying key and report the unsatisfied policy as before."""
import numpy as np
import pytest

import share_cases as sc
import test_bsw07_encrypt_gpu as bg
import test_lw11_encrypt_plan as lp
import test_waters11_encrypt_plan as wp
import bsw07_fixture
import lw11_fixture as lf
import waters11_fixture as wf
from sw05_fixture import kbytes
from test_bsw07_encrypt_plan import fixture_arrays, fixture_inputs
from gopairingbasedcryptography_amd import bsw07, lw11, waters11

pytestmark = pytest.mark.gpu
N = 67


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def kinds(tensors):
    import torch
    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if tensors else (lambda a: np.ascontiguousarray(a))
    back = (lambda t: t.cpu().numpy()) if tensors else np.asarray
    return put, back


def scalar_rows(rows, n):
    return kbytes([x for r in rows for x in r]).reshape(n, -1, 32)


# ------------------------------------------------------------------------------------------------ Waters11
@pytest.fixture(scope="module")
def w11(eng):
    shapes, key_attrs = wf.small_policies()
    policies = [shapes[j % 4] for j in range(N)]
    inst = wf.Instance(eng, key_attrs, policies)
    return inst, wp.fixture_inputs(inst)


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_waters11_encrypt_then_decrypt(eng, w11, tensors):
    import torch
    inst, f = w11
    put, back = kinds(tensors)
    msgs = np.asarray(inst.msgs).reshape(N, 384)
    got = waters11.encrypt_batch(eng, f["g1a"], f["e_alpha"], f["h"], inst.policies, put(msgs), put(kbytes(f["s"]).reshape(N, 32)), put(scalar_rows(f["v"], N)), put(scalar_rows(f["r"], N)))
    assert all(tensors == isinstance(g, torch.Tensor) for g in got)
    wp.check_ciphertexts(inst, got, back)
    sat = inst.satisfied()
    assert sat == [j % 4 != 3 for j in range(N)]
    want = msgs * np.array(sat, dtype=np.uint8).reshape(N, 1)
    for msm in (False, True):
        out, ok = waters11.decrypt_batch(eng, inst.key, inst.policies, *got, msm=msm)
        assert back(ok).tolist() == [int(v) for v in sat] and back(out).tobytes() == want.tobytes()


def test_waters11_table_built_once_and_keygen(eng, w11):
    inst, f = w11
    msgs = np.asarray(inst.msgs).reshape(N, 384)
    table = waters11.encrypt_table(eng, f["g1a"], f["h"])
    try:
        got = waters11.encrypt_batch(eng, f["g1a"], f["e_alpha"], f["h"], inst.policies, msgs, f["s"], f["v"], f["r"], table=table)
        wp.check_ciphertexts(inst, got)
        users = [inst.key_attrs, [500, 11], []] + [[999]] * 64
        t = [wf.sc("t")] + [wf.sc("t", j) for j in range(1, N)]
        K, L, kx, attrs = waters11.keygen_batch(eng, f["g1_alpha"], f["g1a"], f["h"], users, t, table=table)
    finally:
        table.close()
    assert K.shape == (N, 64) and L.shape == (N, 128) and kx.shape == (N, len(inst.key_attrs), 64)
    assert K[0].tobytes() == inst.key[0].tobytes() and L[0].tobytes() == inst.key[1].tobytes()
    assert all(kx[0, i].tobytes() == inst.key[2][u].tobytes() for i, u in enumerate(inst.key_attrs)) and attrs[0].tolist() == inst.key_attrs
    a, alpha = wf.sc("a"), wf.sc("alpha")
    g1 = np.frombuffer(wp.o.g1_to_bytes(wp.o.G1_GEN), dtype=np.uint8)
    assert K.tobytes() == np.asarray(eng.g1_scalar_mul(g1, kbytes([(alpha + a * tj) % wp.R for tj in t]))).tobytes()
    assert kx[1, :2].tobytes() == np.asarray(eng.g1_scalar_mul(g1, kbytes([wf.sc("tau", u) * t[1] % wp.R for u in (11, 500)]))).tobytes()
    assert not kx[1, 2:].any() and not kx[2].any() and attrs[2].tolist() == [-1] * len(inst.key_attrs)
    key = (K[0], L[0], {int(u): kx[0, i] for i, u in enumerate(attrs[0])})
    out, ok = waters11.decrypt_batch(eng, key, inst.policies, *got)
    assert ok.tolist() == [int(j % 4 != 3) for j in range(N)] and out[0].tobytes() == msgs[0].tobytes()


# ------------------------------------------------------------------------------------------------ LW11
@pytest.fixture(scope="module")
def l11(eng):
    m, rho = lf.threshold_policy(3, 5)
    inst = lf.Instance(eng, m, rho, [200, 202, 203], n_ct=N)
    return inst, lp.fixture_inputs(inst)


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_lw11_encrypt_then_decrypt(eng, l11, tensors):
    import torch
    inst, f = l11
    put, back = kinds(tensors)
    msgs = np.asarray(inst.msgs).reshape(N, 384)
    got = lw11.encrypt_batch(eng, f["e"], f["egg_alpha"], f["g2_y"], inst.matrix, inst.rho, put(msgs), put(kbytes(f["s"]).reshape(N, 32)), put(scalar_rows(f["v"], N)),
                             put(scalar_rows(f["w"], N)), put(scalar_rows(f["r"], N)))
    for g, w, shape in zip(got, (inst.c0, inst.c1, inst.c2, inst.c3), ((N, 384), (N, 5, 384), (N, 5, 128), (N, 5, 128))):
        assert tuple(g.shape) == shape and tensors == isinstance(g, torch.Tensor) and back(g).tobytes() == np.asarray(w).tobytes()
    rows, w = lw11.reconstruction_weights(inst.matrix, inst.rho, inst.user_attrs)
    folded = lw11.fold_key(eng, rows, w, inst.h_gid, inst.k_by_row)
    assert back(lw11.decrypt_batch(eng, folded, *got)).tobytes() == msgs.tobytes()
    assert back(lw11.decrypt_batch_msm(eng, folded, inst.h_gid, *got)).tobytes() == msgs.tobytes()
    assert lw11.reconstruction_weights(inst.matrix, inst.rho, [200, 203]) is None                  # two of the five: no key, as before


# ------------------------------------------------------------------------------------------------ BSW07 with tables
@pytest.fixture(scope="module", params=list(bg.POLICIES))
def b07(eng, request):
    make, held, _ = bg.POLICIES[request.param]
    inst = bsw07_fixture.Instance(eng, make(), user_attrs=held, n_ct=N)
    return request.param, inst, fixture_inputs(inst, N)


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_bsw07_tables_is_the_default_route(eng, b07, tensors):
    import torch
    name, inst, (s, coeffs, h, h1) = b07
    put, back = kinds(tensors)
    L = len(bsw07.share_plan(inst.tree)[1])
    msgs = np.stack(inst.msgs)
    args = (put(msgs), put(sc.rows(s).reshape(N, 32)), put(sc.rows([v for q in coeffs for v in q]).reshape(N, -1, 32)))
    plain = bsw07.encrypt_batch(eng, inst.tree, h, inst.e_alpha, h1, *args)
    got = bsw07.encrypt_batch(eng, inst.tree, h, inst.e_alpha, h1, *args, tables=True)
    for g, p, w, shape in zip(got, plain, fixture_arrays(inst), ((N, 384), (N, 64), (N, L, 64), (N, L, 64))):
        assert tuple(g.shape) == shape and tensors == isinstance(g, torch.Tensor) and back(g).tobytes() == w.tobytes() == back(p).tobytes()
    plan = bsw07.decrypt_plan(inst.tree, inst.user_attrs)
    assert plan is not None and bsw07.decrypt_plan(inst.tree, set(bg.POLICIES[name][2])) is None
    folded = bsw07.fold_key(eng, plan, inst.dj, inst.dj_prime)
    cols = [i - 1 for i in folded[0]]
    c_tilde, c, cy, cy_prime = got
    pick = (lambda a: a[:, cols].contiguous()) if tensors else (lambda a: np.ascontiguousarray(a[:, cols]))
    out = bsw07.decrypt_batch_arrays(eng, folded, inst.D, c_tilde, c, pick(cy), pick(cy_prime))
    assert back(out).tobytes() == msgs.tobytes()
