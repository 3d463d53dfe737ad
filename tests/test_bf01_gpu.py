"""Boneh-Franklin BasicIdent on the MI355X (run with -m gpu): the instance of tests/test_bf01_plan.py at n = 16 through bf01.py on the
real engine, host arrays and CUDA tensors — every output byte-equal to the oracle's, which computes in the reference's order (pair,
then gt_exp, then bytes: tests/bf01_fixture.py); one-key and per-item-key Decrypt agree; on the CUDA path every output is a CUDA
tensor."""
import numpy as np
import pytest

from bf01_fixture import Instance, flat_messages
from sw05_fixture import kbytes
from gopairingbasedcryptography_amd import bf01, rng

pytestmark = pytest.mark.gpu
N = 16
SEED = bytes((13 * i + 1) % 256 for i in range(32))


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


@pytest.fixture(scope="module")
def inst(oracle):
    return Instance(oracle, N)


def dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.array(a, copy=True))
    return (t.to(dtype) if dtype is not None else t).cuda()


def same(got, want, cuda=False):
    import torch
    if cuda:
        assert isinstance(got, torch.Tensor) and got.is_cuda
        got = got.cpu().numpy()
    else:
        assert isinstance(got, np.ndarray)
    want = np.asarray(want)
    if got.dtype != np.uint8:
        got, want = got.view(np.uint32), want.view(np.uint32)
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def test_host_arrays(eng, inst):
    assert same(bf01.identities_to_g2(eng, inst.ids), inst.qids) and same(bf01.public_params(eng, inst.x), inst.g1x)
    assert same(bf01.keygen_batch(eng, inst.x, ids=inst.ids), inst.sk)
    c1, (c2, off), c2_len = bf01.encrypt_batch(eng, inst.g1x, inst.msgs, inst.r, ids=inst.ids)
    assert same(c1, inst.c1) and same(c2, inst.c2_data) and same(off, inst.off) and same(c2_len, inst.c2_len)
    m, lens = bf01.decrypt_batch(eng, inst.sk, c1, (c2, off))
    assert same(m, inst.dec_data) and same(lens, inst.c2_len) and m.tobytes() == b"".join(inst.recovered())
    # one identity, one key, sixteen ciphertexts: the fixed-Q pairing and the per-item pairing give the same bytes
    q0 = np.tile(inst.qids[0], (N, 1))
    c1, c2, _ = bf01.encrypt_batch(eng, inst.g1x, inst.data, inst.r, qids=q0, msg_off=inst.off)
    one, lens1 = bf01.decrypt_batch(eng, inst.sk[0], c1, c2, inst.off)
    each, lens2 = bf01.decrypt_batch(eng, np.tile(inst.sk[0], (N, 1)), c1, c2, inst.off)
    assert same(one, inst.dec_data) and same(each, inst.dec_data) and same(lens1, inst.c2_len) and same(lens2, inst.c2_len)


def test_cuda_tensors(eng, inst):
    import torch
    data, off, r, sk, qids = dev(inst.data), dev(inst.off, torch.int64), dev(kbytes(inst.r).reshape(N, 32)), dev(inst.sk), dev(inst.qids)
    ids, ids_off = flat_messages(inst.id_bytes)
    assert same(bf01.identities_to_g2(eng, dev(ids), dev(ids_off, torch.int64)), inst.qids, True)      # identities hashed where they live
    assert same(bf01.keygen_batch(eng, inst.x, qids=qids), inst.sk, True)
    c1, c2, c2_len = bf01.encrypt_batch(eng, inst.g1x, data, r, qids=qids, msg_off=off)
    assert same(c1, inst.c1, True) and same(c2, inst.c2_data, True) and same(c2_len, inst.c2_len, True)
    c1b, c2b, _ = bf01.encrypt_batch(eng, inst.g1x, data, r, ids=inst.ids, msg_off=off)                # host identities beside device messages
    assert same(c1b, inst.c1, True) and same(c2b, inst.c2_data, True)
    m, lens = bf01.decrypt_batch(eng, sk, c1, c2, off)
    assert same(m, inst.dec_data, True) and same(lens, inst.c2_len, True)
    q0 = qids[:1].expand(N, 128).contiguous()
    c1, c2, _ = bf01.encrypt_batch(eng, inst.g1x, data, r, qids=q0, msg_off=off)
    one, lens1 = bf01.decrypt_batch(eng, sk[0], c1, c2, off)
    each, lens2 = bf01.decrypt_batch(eng, sk[:1].expand(N, 128).contiguous(), c1, c2, off)
    assert same(one, inst.dec_data, True) and same(each, inst.dec_data, True) and same(lens1, inst.c2_len, True) and same(lens2, inst.c2_len, True)
    # rows of one width, in and out as [n, 32] tensors
    rows = dev(np.stack([np.frombuffer(m[:32].ljust(32, b"\x07"), dtype=np.uint8) for m in inst.msgs]))
    c1, c2, c2_len = bf01.encrypt_batch(eng, inst.g1x, rows, r, qids=qids)
    assert tuple(c2.shape) == (N, 32) and c2.is_cuda and c2_len.cpu().tolist() == [32] * N
    back, _ = bf01.decrypt_batch(eng, sk, c1, c2)
    assert back.is_cuda and torch.equal(back, rows)


def test_seeded_on_the_device(eng, inst):
    """one draw, stream 0: the ciphertexts are encrypt_batch's on fr_random's scalars, host and CUDA alike, and decrypt"""
    import torch
    data, off, qids, sk = dev(inst.data), dev(inst.off, torch.int64), dev(inst.qids), dev(inst.sk)
    rnd = rng.Randomness(eng, SEED)
    c1, c2, c2_len = bf01.encrypt_batch_seeded(eng, inst.g1x, data, rnd, qids=qids, msg_off=off)
    assert rnd.next_stream == 1 and c1.is_cuda and c2.is_cuda and c2_len.is_cuda
    drawn = eng.fr_random(SEED, N, stream=0)
    want = bf01.encrypt_batch(eng, inst.g1x, inst.data, drawn, qids=inst.qids, msg_off=inst.off)
    assert same(c1, want[0], True) and same(c2, want[1], True) and same(c2_len, want[2], True)
    m, _ = bf01.decrypt_batch(eng, sk, c1, c2, off)
    assert same(m, inst.dec_data, True)
