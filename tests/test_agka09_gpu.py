"""The ASBB planner agka09.py on the MI355X (run with -m gpu): one round trip at n = 8 with group = 4 — keygen, sign, verify_each,
verify_batch, aggregate, encrypt, decrypt — on CUDA tensors and on host arrays, the first key and signature held against
gka/agka09/asbb.go restated in Python integers (oracle/bn254_py.py), and aggregation under validate=True with one R off the subgroup
and one A that is cyclotomic but not of order r."""
import numpy as np
import pytest

import bn254_py as o
import member_cases as mc
from gopairingbasedcryptography_amd import agka09
from gopairingbasedcryptography_amd.rng import Randomness

pytestmark = pytest.mark.gpu
N, GROUP = 8, 4
SEED = bytes(range(60, 92))
STRING = b"one string for every member"


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_round_trip(eng):
    import torch
    r = [0x1000 + 7919 * i for i in range(N)]
    x = [0x2000 + 104729 * i for i in range(N)]
    R, A, X = agka09.keygen_batch(eng, r, x)
    # the reference's KeyGen and Sign for member 0, in Python integers
    X0 = o.g1_mul(o.G1_GEN, x[0])
    H = o.hash_to_g1(STRING, agka09.DST_BYTES_G1)
    assert R[0].tobytes() == o.g2_to_bytes(o.g2_mul(o.G2_GEN, (-r[0]) % o.R)) and X[0].tobytes() == o.g1_to_bytes(X0)
    assert A[0].tobytes() == o.gt_to_bytes(o.pair([X0], [o.G2_GEN]))
    sig = agka09.sign_batch(eng, r, X, strings=[STRING] * N)                               # every member signs the one string
    assert sig[0].tobytes() == o.g1_to_bytes(o.g1_add(X0, o.g1_mul(H, r[0])))
    assert (agka09.verify_each(eng, R, A, sig, strings=[STRING] * N) == 1).all()
    assert (eng.g2_is_in_subgroup(R) == 1).all() and (eng.gt_is_in_subgroup(A) == 1).all() and (eng.g1_is_on_curve(sig) == 1).all()

    # one member signs n strings: verify_batch == verify_each, all valid and with forgeries, on tensors and on host arrays
    strings = [b"string %d" % i for i in range(N)]
    hashed = agka09.hash_strings(eng, strings)
    mine = agka09.sign_batch(eng, [r[2]], X[2], hashed=hashed)
    forged = np.array(mine, copy=True)
    forged[1], forged[6] = mine[2], mine[5]
    want = np.array([0 if i in (1, 6) else 1 for i in range(N)], dtype=np.uint8)
    dR, dA, dh = to_dev(R[2]), to_dev(A[2]), to_dev(hashed)
    for s, w in ((mine, np.ones(N, dtype=np.uint8)), (forged, want)):
        each = agka09.verify_each(eng, dR, dA, to_dev(s), hashed=dh)
        assert each.is_cuda and each.dtype == torch.uint8 and each.cpu().numpy().tolist() == w.tolist()
        got = agka09.verify_batch(eng, dR, dA, to_dev(s), Randomness(eng, SEED), hashed=dh, group=GROUP)
        assert got.is_cuda and got.cpu().numpy().tolist() == w.tolist()
        host = agka09.verify_batch(eng, R[2], A[2], s, Randomness(eng, SEED), strings=strings, group=GROUP)
        assert isinstance(host, np.ndarray) and host.tolist() == w.tolist()

    # aggregate two groups of four, encrypt under each aggregated key, decrypt with the aggregated signature
    seg = [0, 4, 8]
    aR, aA = agka09.aggregate_public_keys(eng, to_dev(R), to_dev(A), seg)
    asig = agka09.aggregate_signatures(eng, to_dev(sig), seg)
    assert aR.is_cuda and tuple(aR.shape) == (2, 128) and tuple(aA.shape) == (2, 384) and tuple(asig.shape) == (2, 64)
    assert agka09.verify_each(eng, aR, aA, asig, strings=[STRING] * 2).cpu().numpy().tolist() == [1, 1]
    assert agka09.verify_each(eng, aR, aA, to_dev(sig[:2]), strings=[STRING] * 2).cpu().numpy().tolist() == [0, 0]
    m = to_dev(eng.gt_exp(A[:2], [5, 9]))                                                  # two plaintexts in GT
    c1, c2, c3 = agka09.encrypt_batch_seeded(eng, aR, aA, m, Randomness(eng, SEED))
    back = agka09.decrypt_batch(eng, c1, c2, c3, asig, strings=[STRING] * 2)
    assert back.is_cuda and bool((back == m).all()) and not bool((c3 == m).all())
    h1, h2, h3 = agka09.encrypt_batch(eng, aR.cpu().numpy(), aA.cpu().numpy(), m.cpu().numpy(), eng.fr_random(SEED, 2, stream=0))
    assert (h1.tobytes(), h2.tobytes(), h3.tobytes()) == tuple(c.cpu().numpy().tobytes() for c in (c1, c2, c3))
    assert agka09.decrypt_batch(eng, h1, h2, h3, asig.cpu().numpy(), strings=[STRING] * 2).tobytes() == m.cpu().numpy().tobytes()
    torch.cuda.synchronize()


def test_aggregation_with_validation(eng):
    """key 1 comes with an R off the subgroup, key 6 with an A that is cyclotomic but not of order r: both masked, both groups zero and
    ok = 0, and a third group of honest keys untouched; signatures likewise with one off the curve"""
    import torch
    n = 12
    r, x = [0x3000 + 31 * i for i in range(n)], [0x4000 + 37 * i for i in range(n)]
    R, A, X = agka09.keygen_batch(eng, r, x)
    g2c, gtc, g1c = mc.g2_cases(), mc.gt_cases(), mc.g1_cases()
    R, A = np.array(R, copy=True), np.array(A, copy=True)
    R[1] = g2c.data[g2c.of("off_subgroup")[0]]
    A[6] = gtc.data[gtc.of("easy_part_only")[0]]
    seg = [0, 4, 8, 12]
    want_mask = [0 if i in (1, 6) else 1 for i in range(n)]
    for put in (lambda a: a, to_dev):
        aR, aA, ok, mask = agka09.aggregate_public_keys(eng, put(R), put(A), seg, validate=True)
        host = [v.cpu().numpy() if torch.is_tensor(v) else v for v in (aR, aA, ok, mask)]
        assert host[3].tolist() == want_mask and host[2].tolist() == [0, 0, 1]
        assert not host[0][:2].any() and not host[1][:2].any()
        plain_R, plain_A = agka09.aggregate_public_keys(eng, R[8:], A[8:], [0, 4])
        assert host[0][2].tobytes() == plain_R.tobytes() and host[1][2].tobytes() == plain_A.tobytes()
    # the rejected elements entered no sum: the masked sum of group 0 is the sum of its three honest keys
    clean_R = eng.g2_sum_segments(np.concatenate([R[0:1], R[2:4]]), [0, 3])
    masked = np.array(R[:4], copy=True)
    masked[1] = 0
    assert eng.g2_sum_segments(masked, [0, 4]).tobytes() == clean_R.tobytes()
    sig = np.array(agka09.sign_batch(eng, r, X, strings=[STRING] * n), copy=True)
    sig[9] = g1c.data[g1c.of("y_plus_one")[0]]
    agg, ok, mask = agka09.aggregate_signatures(eng, to_dev(sig), seg, validate=True)
    assert mask.cpu().numpy().tolist() == [0 if i == 9 else 1 for i in range(n)] and ok.cpu().numpy().tolist() == [1, 1, 0]
    assert not bool(agg[2].any()) and agg[0].cpu().numpy().tobytes() == agka09.aggregate_signatures(eng, sig[:4], [0, 4]).tobytes()
    each = agka09.verify_each(eng, to_dev(R[8:]), to_dev(A[8:]), to_dev(sig[8:]), strings=[STRING] * 4, validate=True)
    assert each.cpu().numpy().tolist() == [1, 0, 1, 1]
    with pytest.raises(ValueError):
        agka09.aggregate_signatures(eng, to_dev(sig), [0, 4, 4, 12])
    torch.cuda.synchronize()
