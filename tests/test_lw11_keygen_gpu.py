"""LW11 decentralised ABE end to end on the device (run with -m gpu): authority_setup -> keygen_batch for 33 users with hashed
identifiers -> the existing encrypt_batch -> fold_key + decrypt_batch per user, for the AND / OR policy and for 3 of 5 as Shamir rows
(tests/lw11_fixture.py).  Every user whose attributes satisfy the policy recovers every message; the user that lacks an attribute does
not; one user's key is the oracle's [alpha_i] g1 + [y_i] H(GID), with H(GID) from the Python oracle's hash to curve."""
import numpy as np
import pytest

import bn254_py as o
from lw11_fixture import and_or_policy, sc as fsc, threshold_policy
from sw05_fixture import kbytes
from gopairingbasedcryptography_amd import lw11
from gopairingbasedcryptography_amd.hash_to import DST_STRING_G1

pytestmark = pytest.mark.gpu
U, N_CT, LACKING = 33, 2, 5
# policy -> (matrix and rho, the attributes user LACKING holds: not enough)
POLICIES = {"and-or": (and_or_policy, [11, 44]), "3of5": (lambda: threshold_policy(3, 5), [200, 203])}


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


@pytest.mark.parametrize("policy", list(POLICIES))
def test_setup_keygen_encrypt_decrypt_round_trip(eng, oracle, policy):
    import torch
    make, few = POLICIES[policy]
    matrix, rho = make()
    attrs = sorted(set(rho))
    A, R, C = len(attrs), len(matrix), len(matrix[0])
    dev = lambda a: torch.from_numpy(np.array(a, dtype=np.uint8, copy=True)).cuda()
    g1, g2 = eng.generators()
    e = np.asarray(eng.pair_batch(g1, g2)).reshape(384)
    alpha, y = [fsc(policy + "alpha", a) for a in attrs], [fsc(policy + "y", a) for a in attrs]
    ea, gy = lw11.authority_setup(eng, e, dev(kbytes(alpha)), dev(kbytes(y)))
    assert ea.is_cuda and gy.is_cuda and ea.shape == (A, 384) and gy.shape == (A, 128)
    assert ea.cpu().numpy().tobytes() == np.asarray(oracle.gt_exp(np.tile(e, A), kbytes(alpha))).tobytes()
    assert gy.cpu().numpy().tobytes() == np.asarray(oracle.g2_scalar_mul(g2, kbytes(y), threads=4)).tobytes()

    # KeyGenerate: every user every attribute, except user LACKING
    gids = ["user-%d@example.org" % u for u in range(U)]
    mask = np.ones((U, A), dtype=np.uint8)
    mask[LACKING] = [a in few for a in attrs]
    K = lw11.keygen_batch(eng, gids, dev(kbytes(alpha)), dev(kbytes(y)), mask=dev(mask))
    assert K.is_cuda and K.shape == (U, A, 64)
    K = K.cpu().numpy()
    h_gid = np.asarray(eng.hash_to_g1([g.encode() for g in gids], DST_STRING_G1)).reshape(U, 64)
    u = 7                                                                         # one user's key from the oracle
    hu = np.frombuffer(o.g1_to_bytes(o.hash_to_g1(gids[u].encode(), DST_STRING_G1)), dtype=np.uint8)
    assert hu.tobytes() == h_gid[u].tobytes()
    ga, hy = np.asarray(oracle.g1_scalar_mul(g1, kbytes(alpha), threads=4)).reshape(A, 64), np.asarray(oracle.g1_scalar_mul(hu, kbytes(y), threads=4)).reshape(A, 64)
    for i in range(A):
        assert K[u, i].tobytes() == np.asarray(oracle.g1_sum(np.stack([ga[i], hy[i]]))).tobytes(), i
    assert not K[LACKING][mask[LACKING] == 0].any() and K[LACKING][mask[LACKING] == 1].any(axis=1).all()

    # Encrypt under the policy with the keys authority_setup made
    eah, gyh = ea.cpu().numpy(), gy.cpu().numpy()
    msgs = eng.gt_exp(dev(np.tile(e, (N_CT, 1))), dev(kbytes([fsc(policy + "msg", t) for t in range(N_CT)])))
    sk = lambda tag, *shape: dev(kbytes([fsc(policy + tag, i) for i in range(int(np.prod(shape)))]).reshape(*shape, 32))
    c0, c1, c2, c3 = lw11.encrypt_batch(eng, e, {a: eah[i] for i, a in enumerate(attrs)}, {a: gyh[i] for i, a in enumerate(attrs)}, matrix, rho, msgs,
                                        sk("s", N_CT), sk("v", N_CT, C - 1), sk("w", N_CT, C - 1), sk("r", N_CT, R))
    want = msgs.cpu().numpy().tobytes()

    # Decrypt per user
    for u in range(U):
        held = [a for i, a in enumerate(attrs) if mask[u, i]]
        plan = lw11.reconstruction_weights(matrix, rho, held)
        if u == LACKING:
            assert plan is None                                                     # ... and with someone else's weights the zero rows give no message
            rows, w = lw11.reconstruction_weights(matrix, rho, attrs)
        else:
            rows, w = plan
        folded = lw11.fold_key(eng, rows, w, h_gid[u], {x: K[u, attrs.index(rho[x])] for x in rows})
        out = lw11.decrypt_batch(eng, folded, c0, c1, c2, c3)
        assert (out.cpu().numpy().tobytes() == want) == (u != LACKING), u
