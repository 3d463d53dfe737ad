"""Waters11 SetUp on the MI355X (run with -m gpu) through gopairingbasedcryptography_amd/waters11.py on the GPU engine: the expectations and
the round trip of tests/waters11_setup_cases.py (the oracle on the known secrets; a universe of 5, a 3-row policy, 2 users) on CUDA
tensors and on host arrays, the gt_table form, the universe cases, and the seeded form against the plain one."""
import numpy as np
import pytest

from sw05_fixture import kbytes
from waters11_setup_cases import A, ALPHA, G1, G2, SEED, TAU, UNIVERSE, check, expected, round_trip
from gopairingbasedcryptography_amd import waters11
from gopairingbasedcryptography_amd.rng import Randomness

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def back(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def test_setup_is_the_oracle_on_the_secrets(oracle, eng):
    want = expected(oracle, UNIVERSE, TAU)
    pp, msk = waters11.setup(eng, UNIVERSE, dev(kbytes([ALPHA])), dev(kbytes([A])), dev(kbytes(TAU)))
    assert msk["g1_alpha"].is_cuda
    check(pp, msk, want, back)
    hpp, hmsk = waters11.setup(eng, UNIVERSE, ALPHA, A, TAU)                   # host arrays, Python integers
    assert isinstance(hmsk["g1_alpha"], np.ndarray)
    check(hpp, hmsk, want)
    gt_table = eng.GTFixedBase(np.asarray(oracle.pair_batch(G1, G2)).reshape(1, 384))
    try:
        check(*waters11.setup(eng, UNIVERSE, dev(kbytes([ALPHA])), dev(kbytes([A])), dev(kbytes(TAU)), gt_table=gt_table), want, back)
    finally:
        gt_table.close()
    check(*waters11.setup(eng, [], dev(kbytes([ALPHA])), dev(kbytes([A])), dev(np.zeros(0, np.uint8))), expected(oracle, [], []), back)
    check(*waters11.setup(eng, [9], ALPHA, A, TAU[:1]), expected(oracle, [9], TAU[:1]))
    with pytest.raises(ValueError, match="distinct integers"):
        waters11.setup(eng, [3, 7, 3], ALPHA, A, TAU[:3])


def test_setup_seeded_is_setup_on_the_draws(eng):
    import torch
    like = torch.zeros(0, dtype=torch.uint8, device="cuda")
    rng = Randomness(eng, SEED)
    pp, msk = waters11.setup_seeded(eng, UNIVERSE, rng, like=like)
    again = Randomness(eng, SEED)
    want_pp, want_msk = waters11.setup(eng, UNIVERSE, again.scalars(like, 1), again.scalars(like, 1), again.scalars(like, 5))
    assert rng.next_stream == 3 and msk["g1_alpha"].is_cuda and torch.equal(msk["g1_alpha"], want_msk["g1_alpha"])
    assert pp["g1a"].tobytes() == want_pp["g1a"].tobytes() and pp["e_alpha"].tobytes() == want_pp["e_alpha"].tobytes()
    assert sorted(pp["h"]) == sorted(UNIVERSE) and all(pp["h"][u].tobytes() == want_pp["h"][u].tobytes() for u in UNIVERSE)


def test_round_trip_from_setup(oracle, eng):
    round_trip(eng, oracle, put=dev, back=back)
    round_trip(eng, oracle)
