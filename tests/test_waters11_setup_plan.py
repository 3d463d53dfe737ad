"""Waters11 SetUp (gopairingbasedcryptography_amd/waters11.py: setup, setup_seeded, universe_range) over the stand-in engine, without a GPU,
on arrays and on CPU tensors: g1a = [a] g1, g1_alpha = [alpha] g1, e_alpha = e(g1, g2)^alpha and h_u = [tau_u] g1 from the oracle on the known
secrets; the gt_table form the same bytes; the empty universe, one attribute, unsorted input with tau in ascending attribute order,
duplicates refused before the engine is touched; universe_range's edges; the seeded form's draws; and a round trip on a universe of 5, a
3-row policy and 2 users through keygen_batch, encrypt_batch and decrypt_batch, one user satisfying the policy and one not."""
import numpy as np
import pytest

from standin_afp25 import SchemeStandIn, Untouchable
from standin_engine import TensorEngine, same_on_tensors, tensors
from sw05_fixture import kbytes, kints
from waters11_setup_cases import A, ALPHA, G1, G2, SEED, TAU, UNIVERSE, check, expected, round_trip
from gopairingbasedcryptography_amd import waters11
from gopairingbasedcryptography_amd.rng import Randomness


@pytest.fixture(scope="module")
def eng(oracle):
    return SchemeStandIn(oracle)


def test_setup_is_the_oracle_on_the_secrets(oracle, eng):
    want = expected(oracle, UNIVERSE, TAU)
    pp, msk = waters11.setup(eng, UNIVERSE, ALPHA, A, TAU)
    check(pp, msk, want)
    assert pp["h"][3].tobytes() == np.asarray(oracle.g1_scalar_mul(G1, kbytes([TAU[0]]))).tobytes()         # ascending order: 3 takes tau[0], 40 tau[4]
    assert pp["h"][40].tobytes() == np.asarray(oracle.g1_scalar_mul(G1, kbytes([TAU[4]]))).tobytes()
    gt_table = eng.GTFixedBase(np.asarray(oracle.pair_batch(G1, G2)).reshape(1, 384))
    tabled, _ = waters11.setup(eng, UNIVERSE, ALPHA, A, TAU, gt_table=gt_table)
    assert tabled["e_alpha"].tobytes() == pp["e_alpha"].tobytes() and gt_table.calls == [(1, 1, 1)]
    tpp, tmsk = waters11.setup(TensorEngine(eng), UNIVERSE, *tensors(kbytes([ALPHA]), kbytes([A]), kbytes(TAU)))
    check(tpp, tmsk, want, back=lambda t: t.numpy())
    assert same_on_tensors(tmsk["g1_alpha"], np.asarray(msk["g1_alpha"]))
    check(*waters11.setup(eng, [], ALPHA, A, []), expected(oracle, [], []))                                  # the empty universe
    check(*waters11.setup(eng, [9], ALPHA, A, TAU[:1]), expected(oracle, [9], TAU[:1]))                      # one attribute
    check(*waters11.setup(eng, waters11.universe_range(5, 8), ALPHA, A, TAU[:3]), expected(oracle, [5, 6, 7], TAU[:3]))


def test_refusals_come_before_the_engine():
    off = Untouchable()
    for universe, tau in (([3, 7, 3], TAU[:3]), ([-1, 2], TAU[:2]), ([1 << 63], TAU[:1])):
        with pytest.raises(ValueError, match="distinct integers"):
            waters11.setup(off, universe, ALPHA, A, tau)
        rng = Randomness(off, SEED)
        with pytest.raises(ValueError, match="distinct integers"):
            waters11.setup_seeded(off, universe, rng)
        assert rng.next_stream == 0
    for universe in ([3.7, 5], [3.0, 5], [True, 5], ["3", 5]):                  # integers, not what int() would make of them
        with pytest.raises(ValueError, match="distinct integers"):
            waters11.setup(off, universe, ALPHA, A, TAU[:2])
    with pytest.raises(ValueError):
        waters11.setup(off, UNIVERSE, ALPHA, A, TAU[:4])                       # a tau per attribute
    assert waters11.universe_range(np.int64(4), np.int64(6)) == [4, 5]
    for start, end in ((2.5, 4), (1, 4.0), (True, 3)):
        with pytest.raises(ValueError, match="must be integers"):
            waters11.universe_range(start, end)
    assert waters11.universe_range(3, 3) == [] and waters11.universe_range(0, 1) == [0] and waters11.universe_range(4, 7) == [4, 5, 6]
    assert waters11.universe_range((1 << 63) - 2, 1 << 63) == [(1 << 63) - 2, (1 << 63) - 1]
    with pytest.raises(ValueError, match="end must be greater than start"):
        waters11.universe_range(5, 4)
    for start, end in ((-1, 3), ((1 << 63) - 1, (1 << 63) + 1)):
        with pytest.raises(ValueError, match="integers in"):
            waters11.universe_range(start, end)


def test_setup_seeded_draws_alpha_a_tau(eng):
    del eng.draws[:]
    rng = Randomness(eng, SEED)
    pp, msk = waters11.setup_seeded(eng, UNIVERSE, rng)
    assert eng.draws == [(1, 0, 0), (1, 1, 0), (5, 2, 0)] and rng.next_stream == 3
    again = Randomness(eng, SEED)
    none = np.zeros(0, np.uint8)
    alpha, a, tau = again.scalars(none, 1), again.scalars(none, 1), again.scalars(none, 5)
    want_pp, want_msk = waters11.setup(eng, UNIVERSE, alpha, a, tau)
    assert pp["g1a"].tobytes() == want_pp["g1a"].tobytes() and pp["e_alpha"].tobytes() == want_pp["e_alpha"].tobytes()
    assert all(pp["h"][u].tobytes() == want_pp["h"][u].tobytes() for u in UNIVERSE) and msk["g1_alpha"].tobytes() == want_msk["g1_alpha"].tobytes()
    assert kints(tau) != sorted(kints(tau))                                    # the check above distinguishes the orders
    del eng.draws[:]
    rng = Randomness(eng, SEED)
    epp, _ = waters11.setup_seeded(eng, [], rng)                               # an empty universe: two streams
    assert eng.draws == [(1, 0, 0), (1, 1, 0)] and rng.next_stream == 2 and epp["h"] == {} and epp["g1a"].tobytes() == pp["g1a"].tobytes()
    like, = tensors(none)
    tpp, tmsk = waters11.setup_seeded(TensorEngine(eng), UNIVERSE, Randomness(TensorEngine(eng), SEED), like=like)
    assert same_on_tensors(tmsk["g1_alpha"], np.asarray(msk["g1_alpha"])) and tpp["g1a"].tobytes() == pp["g1a"].tobytes()


def test_round_trip_from_setup(oracle, eng):
    round_trip(eng, oracle)
