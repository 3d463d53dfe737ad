"""SW05 KeyGenerate of both universes on the MI355X (run with -m gpu) through gopairingbasedcryptography_amd/sw05.py: keygen_batch and
keygen_batch_large on the GPU engine, host arrays and CUDA tensors, reproduce sw05_fixture.Instance.key byte for byte (d = 1, 4, 16,
small and full-size attribute values); three users at once are three single-user calls; and the existing decrypt_batch /
decrypt_batch_large with the generated key return the fixture's messages for the decryptable ciphertexts, ok = 0 for the others."""
import numpy as np
import pytest

import bn254_py as o
from sw05_fixture import Instance, at_size_attributes, sc
from test_sw05_keygen_plan import three_users
from gopairingbasedcryptography_amd import sw05

pytestmark = pytest.mark.gpu
R = o.R
N_UNIV = 12


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def rows(m):
    return np.frombuffer(b"".join((v % R).to_bytes(32, "little") for r in m for v in r), dtype=np.uint8).reshape(len(m), -1, 32).copy()


@pytest.mark.parametrize("large", [False, True], ids=["small", "large"])
@pytest.mark.parametrize("d", [1, 4, 16])
def test_generated_key_is_the_fixture_key_and_decrypts(eng, d, large):
    import torch
    key_attrs, cts = at_size_attributes(6, 20, 24, d, every=3)
    tag = "kgg%d" % d
    inst = Instance(eng, d, key_attrs, cts, n_univ=N_UNIV if large else None, tag=tag)
    y, coeffs, attrs = sc(tag + "y"), [[sc(tag + "q", j) for j in range(1, d)]], [key_attrs]
    side = [[sc(tag + "r", k) for k in range(len(key_attrs))]] if large else [[inst.t[a % R] for a in key_attrs]]
    table = eng.FixedBase(inst.table_bases, g2=True) if large else None
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for put, back in ((lambda a: a, np.asarray), (to_dev, lambda t: t.cpu().numpy())):
        args = (y, put(rows(coeffs)) if d > 1 else None, put(rows(attrs)), put(rows(side)))
        if large:
            dk, Dk = sw05.keygen_batch_large(eng, table, N_UNIV, *args)
            assert back(dk).tobytes() == np.asarray(inst.key[1]).tobytes() and back(Dk).tobytes() == np.asarray(inst.key[2]).tobytes()
            key = (key_attrs, back(dk).reshape(-1, 64), back(Dk).reshape(-1, 128))
            out, ok = sw05.decrypt_batch_large(eng, key, d, cts, inst.E, inst.e_pp, inst.e_prime)
        else:
            D = sw05.keygen_batch(eng, *args)
            assert tuple(D.shape) == (1, len(key_attrs), 64) and back(D).tobytes() == np.asarray(inst.key[1]).tobytes()
            out, ok = sw05.decrypt_batch(eng, (key_attrs, back(D).reshape(-1, 64)), d, cts, inst.E, inst.e_prime)
        want = inst.decryptable()
        assert want == [True, True, False, True, True, False] and ok.tolist() == [int(w) for w in want]
        for t, w in enumerate(want):
            assert (out[t] == np.asarray(inst.msgs)[t]).all() if w else not out[t].any(), t
    if table is not None:
        table.close()


def test_three_users_are_three_single_user_calls(eng):
    inst = Instance(eng, 2, [1, 2, 3], [[1, 2, 3]], n_univ=3, tag="kg3u")
    table = eng.FixedBase(inst.table_bases, g2=True)
    attrs, coeffs, side = three_users(4)
    y = sc("y3")
    D = sw05.keygen_batch(eng, y, coeffs, attrs, side)
    dl, Dl = sw05.keygen_batch_large(eng, table, 3, y, coeffs, attrs, side)
    for j in range(3):
        assert sw05.keygen_batch(eng, y, coeffs[j:j + 1], attrs[j:j + 1], side[j:j + 1]).tobytes() == D[j].tobytes()
        a, b = sw05.keygen_batch_large(eng, table, 3, y, coeffs[j:j + 1], attrs[j:j + 1], side[j:j + 1])
        assert a.tobytes() == dl[j].tobytes() and b.tobytes() == Dl[j].tobytes()
    q = (y + sum(c * pow(attrs[1][2], i + 1, R) for i, c in enumerate(coeffs[1]))) % R
    assert D[1, 2].tobytes() == eng.g1_scalar_mul_base([q * pow(side[1][2], -1, R) % R]).tobytes()
    table.close()
