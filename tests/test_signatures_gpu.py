"""The signature planners bls01.py, zss04.py and bb04sig.py on the MI355X (run with -m gpu), n = 70 signatures per scheme:

  * the bytes of sign_batch equal the oracle's restatement of the reference's Sign for the first 4 items (tests/signatures_fixture.py);
  * verify_batch == verify_each, byte for byte, with forgeries at 0, 7, 8 and 69 and group in {1, 8, 70}, on CUDA tensors (tensors in,
    tensors out) and once on host arrays;
  * seeded BB04 signing is reproducible from the seed, and its r is the generator's stream 0."""
import numpy as np
import pytest

import signatures_fixture as sf
from gopairingbasedcryptography_amd import bb04sig, bls01, zss04
from gopairingbasedcryptography_amd.rng import Randomness

pytestmark = pytest.mark.gpu
N = 70
FORGED = [0, 7, 8, 69]
SEED = bytes(range(100, 132))


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def signed(eng, oracle, scheme):
    """(adapter, key, msg, sig) on the host: N signatures made by the planner's sign_batch, the first 4 held against the oracle"""
    ref = sf.Instance(oracle, scheme, 4)
    if scheme == "zss04":
        msgs = [sf.message(i) for i in range(N)]
        key = [zss04.keygen_batch(eng, [ref.x])[0]]
        msg = zss04.message_scalars(eng, msgs)
        sig = [zss04.sign_batch(eng, ref.x, messages=msgs)]
        assert (zss04.public_params(eng) == ref.eg).all()
    elif scheme == "bb04":
        m, r = [sf.scalar("bb04/m", i) for i in range(N)], [sf.scalar("bb04/r", i) for i in range(N)]
        key = [k[0] for k in bb04sig.keygen_batch(eng, [ref.alpha], [ref.beta])]
        msg = sf.kbytes(m).reshape(N, 32).copy()
        sig = list(bb04sig.sign_batch(eng, ref.alpha, ref.beta, m, r))
    else:
        msgs = [sf.message(i) for i in range(N)]
        key = [bls01.keygen_batch(eng, [ref.x])[0]]
        msg = bls01.hash_messages(eng, msgs)
        sig = [bls01.sign_batch(eng, ref.x, hashed=msg)]
    assert all((k == rk).all() for k, rk in zip(key, ref.key)) and (msg[:4] == ref.msg).all()
    for got, want in zip(sig, ref.sig):
        assert got[:4].tobytes() == want.tobytes()                                         # the reference's Sign, byte for byte
    return ref, key, msg, sig


@pytest.mark.parametrize("scheme", sf.SCHEMES)
def test_verify_batch_equals_verify_each(eng, oracle, scheme):
    import torch
    ref, key, msg, sig = signed(eng, oracle, scheme)
    k, _ = ref.point_sig()
    assert (ref.each(eng, key, msg, sig) == 1).all()                                       # host arrays in, host array out
    forged = [np.array(a, copy=True) for a in sig]
    for p in FORGED:
        forged[k][p] = sig[k][(p + 1) % N]
    want = np.array([0 if i in FORGED else 1 for i in range(N)], dtype=np.uint8)
    dkey, dmsg, dsig = [to_dev(a) for a in key], to_dev(msg), [to_dev(a) for a in forged]
    each = ref.each(eng, dkey, dmsg, dsig)
    assert each.is_cuda and each.dtype == torch.uint8 and (each.cpu().numpy() == want).all()
    for group in (1, 8, 70):
        got = ref.batch(eng, dkey, dmsg, dsig, Randomness(eng, SEED), group)
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == each.shape and bool((got == each).all()), group
    valid = ref.batch(eng, dkey, dmsg, [to_dev(a) for a in sig], Randomness(eng, SEED), 8)
    assert bool((valid == 1).all())
    host = ref.batch(eng, key, msg, forged, Randomness(eng, SEED), 8)
    assert isinstance(host, np.ndarray) and host.tobytes() == want.tobytes()
    torch.cuda.synchronize()


def test_bb04_seeded_signing_is_reproducible(eng, oracle):
    import torch
    alpha, beta = sf.scalar("bb04/alpha"), sf.scalar("bb04/beta")
    m = to_dev(sf.kbytes([sf.scalar("bb04/m", i) for i in range(N)]).reshape(N, 32).copy())
    r1, s1 = bb04sig.sign_batch_seeded(eng, alpha, beta, m, Randomness(eng, SEED))
    r2, s2 = bb04sig.sign_batch_seeded(eng, alpha, beta, m, Randomness(eng, SEED))
    assert r1.is_cuda and s1.is_cuda and bool((r1 == r2).all()) and bool((s1 == s2).all())
    assert bool((r1.reshape(-1) == eng.fr_random(SEED, N, stream=0, like=m).reshape(-1)).all())
    r3, s3 = bb04sig.sign_batch_seeded(eng, alpha, beta, m, Randomness(eng, bytes(32)))
    assert not bool((s3 == s1).all())
    y, z = (k[0] for k in bb04sig.keygen_batch(eng, [alpha], [beta]))
    assert bool((bb04sig.verify_each(eng, y, z, bb04sig.public_params(eng), m.reshape(-1), r1, s1) == 1).all())
    torch.cuda.synchronize()
