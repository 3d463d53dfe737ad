"""SW05 fuzzy IBE batched decryption and computeT on the MI355X (run with -m gpu), through gopairingbasedcryptography_amd/sw05.py.

  * the small instances of tests/test_sw05_plan.py on the GPU engine, host arrays and CUDA tensors: the messages, byte-identical to
    the reference's loop on the oracle;
  * at size: 2^14 ciphertexts of 24 attributes, one key of 32, d = 16, both variants — every 64th ciphertext shares exactly d - 1
    attributes with the key: ok = 0 and an all-zero row for exactly those 256, every other message byte for byte (no sampling), the
    first 1024 rows of Lagrange coefficients against Python's integers, 4 ciphertexts against the reference-shaped oracle decrypt;
  * compute_t for 1024 attributes at n = 16 against the fixture's exponent route."""
import numpy as np
import pytest

import bn254_py as o
import fr_lagrange_cases as lc
from sw05_fixture import Instance, at_size_attributes, kints, sc, t_exponent
from test_sw05_plan import KEY, cts_for
from gopairingbasedcryptography_amd import sw05

pytestmark = pytest.mark.gpu
R = o.R


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(eng, inst, put=lambda a: a):
    if inst.n_univ is None:
        return sw05.decrypt_batch(eng, inst.key, inst.d, inst.ct_attrs, put(inst.E), put(inst.e_prime))
    return sw05.decrypt_batch_large(eng, inst.key, inst.d, inst.ct_attrs, put(inst.E), put(inst.e_pp), put(inst.e_prime))


@pytest.mark.parametrize("large", [False, True])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_small_instances_host_and_device(eng, oracle, d, large):
    inst = Instance(eng, d, KEY, cts_for(d), n_univ=5 if large else None, tag="p%d" % d)
    ref = [inst.reference_shaped_decrypt(oracle, t) for t in range(4)]
    assert ref[2] is None
    for put, back in ((lambda a: a, np.asarray), (lambda a: to_dev(np.asarray(a)), lambda t: t.cpu().numpy())):
        out, ok = run(eng, inst, put)
        out, ok = back(out), back(ok)
        assert ok.tolist() == [1, 1, 0, 1] and not out[2].any()
        for t in (0, 1, 3):
            assert (out[t] == np.asarray(inst.msgs)[t]).all() and (out[t] == ref[t]).all(), t


@pytest.mark.parametrize("large", [False, True])
def test_at_size_2_14(eng, oracle, large):
    import torch
    n, a, n_key, d = 1 << 14, 24, 32, 16
    key_attrs, cts = at_size_attributes(n, a, n_key, d, every=64)
    dev = torch.device("cuda", 0)
    inst = Instance(eng, d, key_attrs, cts, n_univ=a if large else None, dev=dev, tag="size")
    try:
        out, ok = run(eng, inst)
        below = np.arange(n) % 64 == 63
        ok = ok.cpu().numpy()
        assert (ok == (~below).astype(np.uint8)).all() and int((ok == 0).sum()) == 256
        wrong = torch.nonzero((out != inst.msgs.reshape(n, 384)).any(dim=1)).flatten().cpu().numpy()
        print("messages: %d of %d rows differ from the plaintexts (256 are below the threshold)" % (wrong.size, n))
        assert wrong.tolist() == np.nonzero(below)[0].tolist()                                 # every decryptable message, byte for byte
        assert not bool(out[torch.from_numpy(np.nonzero(below)[0]).to(dev)].any())       # and all-zero rows for the others
        # the coefficients of the first 1024 decryptable ciphertexts against Python's integers
        _, cp, _ = sw05.select_common(key_attrs, cts, d)
        good = np.nonzero(~below)[0][:1024]
        sets = [[cts[t][p] for p in cp[t]] for t in good]
        delta = eng.fr_lagrange_basis(to_dev(lc.flat(sets).reshape(-1)), d)
        assert kints(delta.cpu().numpy()) == [lc.basis(S, i, 0) for S in sets for i in S]
        host_out = out.cpu().numpy()
        for t in (0, 1, 62, n - 2):
            assert (host_out[t] == inst.reference_shaped_decrypt(oracle, t)).all(), t
        assert inst.reference_shaped_decrypt(oracle, 63) is None
    finally:
        eng.release_workspaces()


def test_compute_t_1024_attributes(eng):
    """n = 16: attributes inside N = {1 .. 17}, 0, small and full-size values; host rows and CUDA rows"""
    n = 16
    inst = Instance(eng, 1, [1], [[1]], n_univ=n, tag="ct16")
    xs = list(range(0, n + 3)) + [R - 1, R + 4] + [sc("tx", i) for i in range(1024 - (n + 3) - 2)]
    assert len(xs) == 1024
    g2 = eng.generators()[1]
    want = np.asarray(eng.g2_scalar_mul(g2, [t_exponent(inst.taus, n, x % R) for x in xs])).reshape(-1, 128)
    table = eng.FixedBase(inst.table_bases.reshape(-1), g2=True)
    try:
        rows = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype=np.uint8).reshape(-1, 32)      # R + 4 goes in unreduced
        got = sw05.compute_t(eng, table, n, rows)
        assert got.shape == (1024, 128) and (np.asarray(got) == want).all()
        got_dev = sw05.compute_t(eng, table, n, to_dev(rows))
        assert (got_dev.cpu().numpy() == want).all()
    finally:
        table.close()
