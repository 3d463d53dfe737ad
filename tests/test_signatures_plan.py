"""The signature planners bls01.py, zss04.py and bb04sig.py on the CPU: over tests/standin_verify.py — the stand-in engine with
fr_dot_segments and gt_equal restated in integers and bytes — with real oracle pairings, n = 9 signatures per scheme.

  * sign_batch gives the reference's signatures (tests/signatures_fixture.py: the oracle in the reference's order) and verify_each
    accepts them all;
  * verify_batch == verify_each with forgeries at 0, 3, 4 and 8, for group in {1, 4, 9}, with keys, messages and signatures tampered
    in turn, on numpy arrays and on CPU tensors through TensorEngine;
  * the point at infinity as a signature is rejected both ways;
  * the cancellation case: S + D and S - D on one message pass the group equation with weights all 1 — the reason for weights — and
    are both rejected with weights from a Randomness;
  * n = 0; an all-valid batch makes no pair_batch call; zero weights are refused on the host path."""
import numpy as np
import pytest

from standin_engine import GT_ONE, TensorEngine, recorded, tensors
from standin_verify import VerifyStandIn
import signatures_fixture as sf
from gopairingbasedcryptography_amd import _plan, bb04sig, bls01, zss04
from gopairingbasedcryptography_amd.rng import Randomness

N = 9
FORGED = [0, 3, 4, 8]
SEED = bytes(range(32))


@pytest.fixture(scope="module")
def eng(oracle):
    return VerifyStandIn(oracle)


@pytest.fixture(scope="module")
def insts(oracle):
    return {s: sf.Instance(oracle, s, N) for s in sf.SCHEMES}


def host(a):
    return a if isinstance(a, np.ndarray) else a.numpy()


@pytest.mark.parametrize("scheme", sf.SCHEMES)
def test_sign_then_verify_each_accepts_every_signature(eng, insts, scheme):
    """the first check: the reference's Sign, then the reference's Verify per item"""
    inst = insts[scheme]
    if scheme == "zss04":
        sig = [zss04.sign_batch(eng, inst.x, messages=inst.msgs)]
        assert (zss04.public_params(eng) == inst.eg).all() and (zss04.keygen_batch(eng, [inst.x])[0] == inst.key[0]).all()
        assert (zss04.message_scalars(eng, inst.msgs) == inst.msg).all() and max(len(m) for m in inst.msgs) > 64
        assert (zss04.verify_each(eng, inst.key[0], inst.eg, sig[0], messages=inst.msgs) == 1).all()
    elif scheme == "bb04":
        sig = list(bb04sig.sign_batch(eng, inst.alpha, inst.beta, inst.msgs, inst.r))
        y, z = bb04sig.keygen_batch(eng, [inst.alpha], [inst.beta])
        assert (y[0] == inst.key[0]).all() and (z[0] == inst.key[1]).all() and (bb04sig.public_params(eng) == inst.eg).all()
    else:
        sig = [bls01.sign_batch(eng, inst.x, messages=inst.msgs)]
        assert (bls01.keygen_batch(eng, [inst.x])[0] == inst.key[0]).all() and (bls01.public_params(eng) == sf.G1).all()
        assert (bls01.hash_messages(eng, inst.msgs) == inst.msg).all()
        assert (bls01.verify_each(eng, inst.key[0], sf.G1, sig[0], messages=inst.msgs) == 1).all()
    for got, want in zip(sig, inst.sig):
        assert got.shape == want.shape and got.tobytes() == want.tobytes()                # the reference's Sign, byte for byte
    ok = inst.each(eng, inst.key, inst.msg, inst.sig)
    assert ok.dtype == np.uint8 and ok.shape == (N,) and (ok == 1).all()
    per_item = [np.tile(k, (N, 1)) for k in inst.key]                                      # a key per item
    assert (inst.each(eng, per_item, inst.msg, inst.sig) == 1).all()


def test_one_of_gt_is_the_oracles():
    assert _plan.GT_ONE.tobytes() == GT_ONE.tobytes()


@pytest.mark.parametrize("scheme", sf.SCHEMES)
@pytest.mark.parametrize("tamper", ["signatures", "messages", "keys"])
def test_verify_batch_equals_verify_each(eng, insts, scheme, tamper):
    inst = insts[scheme]
    key, msg, sig = inst.key, inst.msg, inst.sig
    if tamper == "signatures":
        sig = inst.forged(FORGED)
    elif tamper == "messages":
        msg = inst.tampered_msg(FORGED)
    else:
        key = inst.other_key
    want = inst.each(eng, key, msg, sig)
    assert want.tolist() == ([0] * N if tamper == "keys" else [0 if i in FORGED else 1 for i in range(N)])
    teng = TensorEngine(eng)
    tkey, (tmsg,), tsig = tensors(*key), tensors(msg), tensors(*sig)
    for group in (1, 4, 9):
        got = inst.batch(eng, key, msg, sig, Randomness(eng, SEED), group)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.tobytes() == want.tobytes(), group
        tgot = inst.batch(teng, tkey, tmsg, tsig, Randomness(teng, SEED), group)
        import torch
        assert isinstance(tgot, torch.Tensor) and tgot.dtype == torch.uint8 and tgot.numpy().tobytes() == want.tobytes(), group
    rho = eng.fr_random(SEED, N, stream=5)                                                 # the caller's rows
    assert inst.batch(eng, key, msg, sig, rho, 4).tobytes() == want.tobytes()


@pytest.mark.parametrize("scheme", sf.SCHEMES)
def test_point_at_infinity_is_rejected_both_ways(eng, insts, scheme):
    inst = insts[scheme]
    k, _ = inst.point_sig()
    sig = [np.array(a, copy=True) for a in inst.sig]
    sig[k][2] = 0
    want = [1, 1, 0] + [1] * (N - 3)
    assert inst.each(eng, inst.key, inst.msg, sig).tolist() == want
    for group in (1, 4, 9):
        assert inst.batch(eng, inst.key, inst.msg, sig, Randomness(eng, SEED), group).tolist() == want


def test_zss04_sign_gives_infinity_when_the_denominator_is_zero(eng, insts):
    inst = insts["zss04"]
    hm = np.array(inst.msg[:2], copy=True)
    hm[1] = np.frombuffer(((-inst.x) % sf.R).to_bytes(32, "little"), dtype=np.uint8)       # H(m) + x = 0
    s = zss04.sign_batch(eng, inst.x, hm=hm)
    assert s[0].tobytes() == inst.sig[0][0].tobytes() and not s[1].any()
    assert zss04.verify_each(eng, inst.key[0], inst.eg, s, hm=hm).tolist() == [1, 0]


@pytest.mark.parametrize("scheme", sf.SCHEMES)
def test_cancellation_is_why_the_weights_are_random(eng, oracle, scheme):
    """items 0 and 1 sign one message; S_0 + D and S_1 - D are both invalid, leave every sum of the group unchanged and pass the group
    equation with weights all 1.  With weights from a Randomness both are rejected."""
    n = 4
    inst = sf.Instance(oracle, scheme, n, same=[(0, 1)])
    k, width = inst.point_sig()
    assert inst.msg[0].tobytes() == inst.msg[1].tobytes()
    d = (sf.g2_mul if width == 128 else sf.g1_mul)(oracle, [7])
    add, sub = (eng.g2_add, eng.g2_sub) if width == 128 else (eng.g1_add, eng.g1_sub)
    sig = [np.array(a, copy=True) for a in inst.sig]
    sig[k][0] = add(inst.sig[k][0], d)[0]
    sig[k][1] = sub(inst.sig[k][1], d)[0]
    want = [0, 0, 1, 1]
    assert inst.each(eng, inst.key, inst.msg, sig).tolist() == want
    ones = np.tile(np.frombuffer((1).to_bytes(32, "little"), dtype=np.uint8), (n, 1))
    seg = _plan.group_table(n, n)
    assert inst.values(eng, inst.key, inst.msg, sig, ones, seg).reshape(-1).tobytes() == GT_ONE.tobytes()      # the group equation passes
    rho = Randomness(eng, SEED).scalars(ones, n)
    assert inst.values(eng, inst.key, inst.msg, sig, rho, seg).reshape(-1).tobytes() != GT_ONE.tobytes()
    for group in (2, 4):
        assert inst.batch(eng, inst.key, inst.msg, sig, Randomness(eng, SEED), group).tolist() == want


@pytest.mark.parametrize("scheme", sf.SCHEMES)
def test_empty_batch(eng, insts, scheme):
    inst = insts[scheme]
    msg, sig = inst.msg[:0], [a[:0] for a in inst.sig]
    rng = Randomness(eng, SEED)
    for out in (inst.each(eng, inst.key, msg, sig), inst.batch(eng, inst.key, msg, sig, rng, 4)):
        assert isinstance(out, np.ndarray) and out.shape == (0,) and out.dtype == np.uint8
    assert rng.next_stream == 0                                                            # nothing was drawn
    if scheme == "zss04":
        assert zss04.sign_batch(eng, inst.x, messages=[]).shape == (0, 64)
    elif scheme == "bb04":
        r, s = bb04sig.sign_batch(eng, inst.alpha, inst.beta, [], [])
        assert r.shape == (0, 32) and s.shape == (0, 64)
    else:
        assert bls01.sign_batch(eng, inst.x, messages=[]).shape == (0, 128)


@pytest.mark.parametrize("scheme", sf.SCHEMES)
def test_all_valid_batch_makes_no_pair_batch_call_and_one_draw(oracle, insts, scheme):
    eng = VerifyStandIn(oracle)
    inst = insts[scheme]
    calls = recorded(eng, ["pair_batch", "multi_pair", "multi_pair_fixed_q", "gt_equal", "fr_dot_segments", "g1_multi_scalar_mul", "g2_multi_scalar_mul", "fr_mul"])
    rng = Randomness(eng, SEED)
    assert (inst.batch(eng, inst.key, inst.msg, inst.sig, rng, 4) == 1).all()
    names = [c[0] for c in calls]
    assert "pair_batch" not in names and names.count("gt_equal") == 1
    assert names.count("fr_dot_segments") == (0 if scheme == "bls01" else 1)               # sum rho_i: BLS01's equation has no such term
    assert eng.draws == [(N, 0, 0)] and rng.next_stream == 1                               # ONE draw, one stream, weight i from index i
    if scheme == "zss04":
        assert names.count("g1_multi_scalar_mul") == 2 and names.count("fr_mul") == 1 and names.count("multi_pair_fixed_q") == 1 and "multi_pair" not in names
        (_, (P, Q)), = [c for c in calls if c[0] == "multi_pair_fixed_q"]
        assert len(Q) == 2 * 128 and len(P) == 3 * 2 * 64                                  # m = 2 over (g2, P), three groups
    elif scheme == "bb04":
        assert names.count("g1_multi_scalar_mul") == 3 and names.count("fr_mul") == 2 and names.count("multi_pair_fixed_q") == 1
        (_, (P, Q)), = [c for c in calls if c[0] == "multi_pair_fixed_q"]
        assert len(Q) == 3 * 128 and len(P) == 3 * 3 * 64
    else:
        assert names.count("g2_multi_scalar_mul") == 2 and names.count("multi_pair") == 1 and "multi_pair_fixed_q" not in names
    # with one forgery only its group goes through the per-item Verify
    calls.clear()
    got = inst.batch(eng, inst.key, inst.msg, inst.forged([5]), Randomness(eng, SEED), 4)
    assert got.tolist() == [1, 1, 1, 1, 1, 0, 1, 1, 1]
    if scheme == "bls01":
        segs = [len(c[1][2]) - 1 for c in calls if c[0] == "multi_pair"]
        assert segs == [3, 4]                                                              # three groups, then the four items of group 1
    else:
        (_, (P, Q)), = [c for c in calls if c[0] == "pair_batch"]
        assert len(P) == 4 * 64


def test_weights_must_be_nonzero_and_group_positive(eng, insts):
    inst = insts["zss04"]
    rho = np.array(eng.fr_random(SEED, N), copy=True)
    rho[3] = np.frombuffer(sf.R.to_bytes(32, "little"), dtype=np.uint8)                    # r itself: zero modulo r
    with pytest.raises(ValueError, match="non-zero"):
        inst.batch(eng, inst.key, inst.msg, inst.sig, rho, 4)
    with pytest.raises(ValueError):
        inst.batch(eng, inst.key, inst.msg, inst.sig, rho[:-1], 4)
    for group in (0, -1, 2.5):
        with pytest.raises(ValueError, match="group"):
            inst.batch(eng, inst.key, inst.msg, inst.sig, Randomness(eng, SEED), group)
