"""The seeded planners on the MI355X (run with -m gpu): bsw07.encrypt_batch_seeded, waters11.encrypt_batch_seeded,
lw11.encrypt_batch_seeded and sw05.keygen_batch_seeded / keygen_batch_large_seeded on the GPU engine, host arrays and CUDA tensors, with
the randomness drawn by the device generator.  Each output is, byte for byte, the existing planner's on the scalars the Python oracle
(tests/chacha_cases.py) gives for the documented streams, and the existing decryptors recover the messages."""
import numpy as np
import pytest

import chacha_cases as cc
import bsw07_fixture
import lw11_fixture as lf
import waters11_fixture as wf
from sw05_fixture import Instance as Sw05Instance
from test_bsw07_encrypt_plan import fixture_inputs as bsw07_inputs
from test_lw11_encrypt_plan import fixture_inputs as lw11_inputs
from test_sw05_keygen_plan import three_users
from test_waters11_encrypt_plan import fixture_inputs as waters11_inputs
from gopairingbasedcryptography_amd import bsw07, lw11, rng, sw05, waters11

pytestmark = pytest.mark.gpu
N = 5
SEED = bytes((11 * i + 5) % 256 for i in range(32))


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


def drawn(stream, *shape):
    """the oracle's scalars of one draw: [*shape, 32] from index 0 of `stream`, row-major"""
    return cc.scalars(SEED, stream, 0, int(np.prod(shape))).reshape(*shape, 32)


def same(got, want, back, tensors):
    import torch
    return all(isinstance(g, torch.Tensor) == tensors and tuple(g.shape) == tuple(w.shape) and back(g).tobytes() == back(w).tobytes() for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ BSW07
@pytest.fixture(scope="module")
def b07(eng):
    L, T = bsw07.Leaf, bsw07.Threshold
    tree = T(2, L(11), T(2, L(22), L(33)), L(44))                                # a 2-of-3 root with one nested 2-of-2 gate
    inst = bsw07_fixture.Instance(eng, tree, user_attrs=[22, 33, 44], n_ct=N)
    _, _, h, h1 = bsw07_inputs(inst, N)
    return inst, h, h1


@pytest.mark.parametrize("tables", [False, True], ids=["plain", "tables"])
@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_bsw07_seeded_encrypt_then_decrypt(eng, b07, tensors, tables):
    inst, h, h1 = b07
    put, back = kinds(tensors)
    msgs = np.stack(inst.msgs)
    r = rng.Randomness(eng, SEED)
    got = bsw07.encrypt_batch_seeded(eng, inst.tree, h, inst.e_alpha, h1, put(msgs), r, tables=tables)
    assert r.next_stream == 2                                                    # s [n], coeffs [n, 2]
    want = bsw07.encrypt_batch(eng, inst.tree, h, inst.e_alpha, h1, put(msgs), put(drawn(0, N)), put(drawn(1, N, 2)), tables=tables)
    assert same(got, want, back, tensors) and [tuple(g.shape) for g in got] == [(N, 384), (N, 64), (N, 4, 64), (N, 4, 64)]
    later = bsw07.encrypt_batch_seeded(eng, inst.tree, h, inst.e_alpha, h1, put(msgs), r, tables=tables)
    assert r.next_stream == 4 and back(later[1]).tobytes() != back(got[1]).tobytes()
    folded = bsw07.fold_key(eng, bsw07.decrypt_plan(inst.tree, inst.user_attrs), inst.dj, inst.dj_prime)
    cols = [i - 1 for i in folded[0]]
    pick = (lambda a: a[:, cols].contiguous()) if tensors else (lambda a: np.ascontiguousarray(a[:, cols]))
    for c_tilde, c, cy, cy_prime in (got, later):
        out = bsw07.decrypt_batch_arrays(eng, folded, inst.D, c_tilde, c, pick(cy), pick(cy_prime))
        assert back(out).tobytes() == msgs.tobytes()


# ------------------------------------------------------------------------------------------------ Waters11
@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_waters11_seeded_encrypt_then_decrypt(eng, tensors):
    shapes, key_attrs = wf.small_policies()
    policies = [shapes[j % 2] for j in range(N)]                                  # two distinct small policies, both satisfied by the key
    inst = wf.Instance(eng, key_attrs, policies)
    f = waters11_inputs(inst)
    put, back = kinds(tensors)
    msgs = np.asarray(inst.msgs).reshape(N, 384)
    pad = waters11.pad_policies(policies)
    R, C = pad.rows, pad.cols
    r = rng.Randomness(eng, SEED)
    got = waters11.encrypt_batch_seeded(eng, f["g1a"], f["e_alpha"], f["h"], policies, put(msgs), r)
    assert r.next_stream == 3                                                    # s [n], v [n, C - 1], r [n, R]
    want = waters11.encrypt_batch(eng, f["g1a"], f["e_alpha"], f["h"], pad, put(msgs), put(drawn(0, N)), put(drawn(1, N, C - 1)), put(drawn(2, N, R)))
    assert same(got, want, back, tensors)
    out, ok = waters11.decrypt_batch(eng, inst.key, policies, *got)
    assert back(ok).tolist() == [1] * N and back(out).tobytes() == msgs.tobytes()


# ------------------------------------------------------------------------------------------------ LW11
@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_lw11_seeded_encrypt_then_decrypt(eng, tensors):
    m, rho = lf.and_or_policy()                                                   # one 4-row policy, 3 columns
    inst = lf.Instance(eng, m, rho, [11, 22, 44, 99], n_ct=N)
    f = lw11_inputs(inst)
    put, back = kinds(tensors)
    msgs = np.asarray(inst.msgs).reshape(N, 384)
    pub = (f["e"], f["egg_alpha"], f["g2_y"], m, rho)
    r = rng.Randomness(eng, SEED)
    got = lw11.encrypt_batch_seeded(eng, *pub, put(msgs), r)
    assert r.next_stream == 4                                                    # s [n], v [n, 2], w [n, 2], r [n, 4]
    want = lw11.encrypt_batch(eng, *pub, put(msgs), put(drawn(0, N)), put(drawn(1, N, 2)), put(drawn(2, N, 2)), put(drawn(3, N, 4)))
    assert same(got, want, back, tensors)
    rows, w = lw11.reconstruction_weights(m, rho, inst.user_attrs)
    folded = lw11.fold_key(eng, rows, w, inst.h_gid, inst.k_by_row)
    assert back(lw11.decrypt_batch(eng, folded, *got)).tobytes() == msgs.tobytes()


# ------------------------------------------------------------------------------------------------ SW05
@pytest.mark.parametrize("tensors", [False, True], ids=["host", "dev"])
def test_sw05_seeded_keys_are_keygen_on_the_oracle_coefficients(eng, tensors):
    """k = 3 users, m = 4 attributes, d = 3, both universes"""
    put, back = kinds(tensors)
    inst = Sw05Instance(eng, 2, [1, 2, 3], [[1, 2, 3]], n_univ=3, tag="kgseed")
    table = eng.FixedBase(inst.table_bases, g2=True)
    R = cc.R
    rows = lambda grid: np.frombuffer(b"".join((v % R).to_bytes(32, "little") for r in grid for v in r), dtype=np.uint8).reshape(len(grid), -1, 32).copy()
    attrs, _, side = three_users(3)
    attrs, side, y, d = put(rows(attrs)), put(rows(side)), 987654321, 3
    try:
        r = rng.Randomness(eng, SEED)
        D = sw05.keygen_batch_seeded(eng, y, d, attrs, side, r)
        assert r.next_stream == 1                                                # coeffs [k, d - 1]
        assert same((D,), (sw05.keygen_batch(eng, y, put(drawn(0, 3, 2)), attrs, side),), back, tensors) and tuple(D.shape) == (3, 4, 64)
        got = sw05.keygen_batch_large_seeded(eng, table, 3, y, d, attrs, r)
        assert r.next_stream == 3                                                # coeffs, then r [k, m]
        assert same(got, sw05.keygen_batch_large(eng, table, 3, y, put(drawn(1, 3, 2)), attrs, put(drawn(2, 3, 4))), back, tensors)
        one = sw05.keygen_batch_seeded(eng, y, 1, attrs, side, r)                # d == 1: no draw
        assert r.next_stream == 3 and same((one,), (sw05.keygen_batch(eng, y, None, attrs, side),), back, tensors)
    finally:
        table.close()
