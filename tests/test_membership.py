"""Membership of in-memory G1, G2 and GT elements on the CPU (include/gpbc_bn254_member.h, csrc/member29.hip.hpp, agka09.py):

  * the lane bodies of the four kernels compiled for the host with -DGPBC_BOUNDS (tools/bounds_check.cpp: hc_g1_is_on_curve,
    hc_g2_is_in_subgroup, hc_gt_is_in_subgroup) on every case of tests/member_cases.py against the oracle's truth.  Under GPBC_BOUNDS every
    product asserts its int64 columns and every normalisation its limbs, for the interval classes of the operands, and a violation aborts:
    a run that finishes is the limb-bound proof.  With force = 1 every GT element — the random, the Miller value, minus one, zero, the
    non-canonical ones loaded as zero — goes through both x^u chains, the Granger-Scott squarings and the product, as a lane pair does on
    the device beside a neighbour that is still a candidate;
  * the header's prototypes against _lib.MEMBER_SIGNATURES, the version entry, the argument errors of the C entries (decided before any
    device is touched) and of the Python entries;
  * the ASBB planner over tests/standin_member.py: the reference's operations in the reference's order, the key homomorphism of
    gka/agka09/asbb.go:21-30 with three members, validation (masks, zero rows, ok = 0, a rejected element replaced by the neutral
    element before the sum), the empty group, verify_batch == verify_each."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT
from bounds_harness import hc  # noqa: F401  (the fixture)
import abi_headers
import bn254_py as o
import member_cases as mc
from standin_engine import TensorEngine, recorded, tensors
from standin_member import MemberStandIn
from gopairingbasedcryptography_amd import _plan, agka09
from gopairingbasedcryptography_amd.rng import Randomness

HEADER = os.path.join(ROOT, "include", "gpbc_bn254_member.h")
GUARD = 0xA5
SEED = bytes(range(32))


# ------------------------------------------------------------------------------------------------ the lane bodies
def verdicts(fn, corpus, *flag):
    ok = np.full(len(corpus) + 16, GUARD, dtype=np.uint8)
    fn(corpus.data.ctypes.data, len(corpus), ok.ctypes.data, *flag)
    assert (ok[len(corpus):] == GUARD).all()
    return ok[:len(corpus)]


def same(corpus, got, truth):
    want = corpus.truth[truth]
    assert got.tolist() == want.tolist(), [(corpus.describe(i), int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0]]


def test_g1_lane_body_on_every_case(hc):
    same(mc.g1_cases(), verdicts(hc.hc_g1_is_on_curve, mc.g1_cases()), "on_curve")


@pytest.mark.parametrize("curve_only,truth", [(1, "on_curve"), (0, "in_subgroup")])
def test_g2_lane_body_on_every_case(hc, curve_only, truth):
    same(mc.g2_cases(), verdicts(hc.hc_g2_is_in_subgroup, mc.g2_cases(), curve_only), truth)


@pytest.mark.parametrize("force", [1, 0])
def test_gt_lane_body_on_every_case(hc, force):
    """force = 1: no element leaves before the chain — the limb-bound proof for values outside the cyclotomic subgroup; force = 0: the
    skip of a wavefront without a candidate (here the pair is the wavefront) changes no verdict.  A verdict of 2 would be two lanes of a
    pair that disagree."""
    c = mc.gt_cases()
    assert {"random", "miller", "minus_one", "zero", "easy_part_only", "coordinate_max"} <= set(c.cls)
    same(c, verdicts(hc.hc_gt_is_in_subgroup, c, force), "in_subgroup")


def test_the_cases_hold_every_class_with_its_truth():
    assert set(mc.g1_cases().cls) == set(mc.G1_CLASSES) and set(mc.g2_cases().cls) == set(mc.G2_CLASSES) and set(mc.gt_cases().cls) == set(mc.GT_CLASSES)
    g2 = mc.g2_cases()
    assert {int(g2.truth["in_subgroup"][i]) for i in g2.of("y2_in_fp")} <= {0, 1}
    # on the twist the identity and the definition agree: nothing is in the subgroup without being on the twist
    assert not (g2.truth["in_subgroup"] & ~g2.truth["on_curve"] & 1).any()
    for corpus, truth in ((mc.g1_cases(), "on_curve"), (g2, "in_subgroup"), (mc.gt_cases(), "in_subgroup")):
        for pattern in ("mixed", "one_bad", "one_good", "all_bad"):
            data, want, idx = mc.tiled(corpus, 65, truth, pattern)
            assert data.shape == (65, corpus.width) and (want == corpus.truth[truth][idx]).all()
            block = 32 if corpus.width == 384 else 64
            if pattern == "one_bad":
                assert int((want[:block] == 0).sum()) == 1
            if pattern == "one_good":
                assert int((want[:block] == 1).sum()) == 1
            if pattern == "all_bad":
                assert not want.any()


# ------------------------------------------------------------------------------------------------ the header, the table, the build
@pytest.fixture(scope="module")
def lib():
    from gopairingbasedcryptography_amd import _build, _lib
    _build.build_library()
    return _lib.load()


def test_member_signature_table_is_the_member_header(lib):
    from gopairingbasedcryptography_amd import _lib
    protos = abi_headers.prototypes("gpbc_bn254_member.h")
    entries = ["gpbc_g1_is_on_curve", "gpbc_g2_is_on_curve", "gpbc_g2_is_in_subgroup", "gpbc_gt_is_in_subgroup"]
    assert sorted(protos) == sorted(_lib.MEMBER_SIGNATURES) == sorted(entries + [e + "_dev" for e in entries] + ["gpbc_member_version"])
    ctype = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int}
    for name, (ret, params) in protos.items():
        assert _lib.MEMBER_SIGNATURES[name] == ret + ":" + "".join(params), name
        fn = getattr(lib, name)                                                            # load() declared it
        assert fn.restype is ctype[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [ctype[k] for k in params], name
    assert lib.gpbc_member_version() == 1 and lib.gpbc_abi_version() == 8
    header = open(HEADER).read()
    assert '#include "gpbc_bn254.h"' in header
    assert all(cite in header for cite in ("zss04_signature_test.go:62,107", "bb04_signature_test.go:35-39,98", "asbb.go:193-220"))


def test_build_lists_cover_the_new_files_and_the_twelfth_unit():
    """the membership kernels have a unit of their own; the pairing and the wire unit, whose headers the lane bodies come from, do not
    know of them (csrc/gpbc_member.hip says why)"""
    from gopairingbasedcryptography_amd import _build
    assert "member29.hip.hpp" in _build.HEADERS and os.path.exists(os.path.join(_build.CSRC, "member29.hip.hpp"))
    assert "gpbc_member.hip" in _build.UNITS
    unit = open(os.path.join(_build.CSRC, "gpbc_member.hip")).read()
    assert all(k in unit for k in ("k_g1_is_on_curve", "k_g2_is_on_curve", "k_g2_is_in_subgroup", "k_gt_is_in_subgroup", '#include "member29.hip.hpp"'))
    for older in ("gpbc_pairing.hip", "gpbc_wire.hip"):
        assert "member" not in open(os.path.join(_build.CSRC, older)).read(), older


def test_c_argument_errors_come_before_any_device(lib):
    """n == 0 is a no-op; a null pointer, an overlap, a misaligned input or too many rows is GPBC_ERR_INVALID_ARG (-1) — decided on the
    arguments alone, so it shows without a GPU"""
    stream = None
    for name, width in (("gpbc_g1_is_on_curve", 64), ("gpbc_g2_is_on_curve", 128), ("gpbc_g2_is_in_subgroup", 128), ("gpbc_gt_is_in_subgroup", 384)):
        host, dev = getattr(lib, name), getattr(lib, name + "_dev")
        buf = np.zeros(4 * width + 8, dtype=np.uint8)
        ok = np.full(4, GUARD, dtype=np.uint8)
        a, k = buf.ctypes.data, ok.ctypes.data
        assert host(None, 0, None) == 0 and dev(None, 0, None, stream) == 0
        for call in (lambda *args: host(*args), lambda *args: dev(*args, stream)):
            assert call(None, 4, k) == -1 and b"null" in lib.gpbc_last_error()
            assert call(a, 4, None) == -1
            assert call(a, 4, a + 4 * width - 1) == -1 and b"overlaps" in lib.gpbc_last_error()       # the last input byte
            assert call(a, 4, a) == -1
            assert call(a + 1, 4, k) == -1 and b"aligned" in lib.gpbc_last_error()
            assert call(a, 1 << 31, k) == -1 and b"too many" in lib.gpbc_last_error()
        assert (ok == GUARD).all()


def test_python_argument_errors():
    from gopairingbasedcryptography_amd import bn254
    assert bn254.g1_is_in_subgroup is bn254.g1_is_on_curve
    for fn, width in ((bn254.g1_is_on_curve, 64), (bn254.g2_is_on_curve, 128), (bn254.g2_is_in_subgroup, 128), (bn254.gt_is_in_subgroup, 384)):
        assert list(inspect.signature(fn).parameters) == ["x", "out"]
        with pytest.raises(ValueError, match="whole number of rows"):
            fn(np.zeros(width - 1, dtype=np.uint8))
        with pytest.raises(ValueError, match="out must be"):
            fn(np.zeros(2 * width, dtype=np.uint8), out=np.zeros(3, dtype=np.uint8))
        with pytest.raises(ValueError, match="out must be"):
            fn(np.zeros(2 * width, dtype=np.uint8), out=np.zeros(2, dtype=np.int32))
        empty = fn(np.zeros(0, dtype=np.uint8))                                             # no engine behind this call
        assert isinstance(empty, np.ndarray) and empty.dtype == np.uint8 and empty.shape == (0,)


# ------------------------------------------------------------------------------------------------ ASBB over the stand-in engine
MEMBERS = 3
STRING = b"the session of 2026-01-13"


def arr(b):
    return np.frombuffer(b, dtype=np.uint8)


@pytest.fixture(scope="module")
def eng(oracle):
    return MemberStandIn(oracle)


class Asbb:
    """gka/agka09/asbb.go in Python integers (oracle/bn254_py.py), the operations in the reference's order: three members' keys, their
    signatures on one string, the aggregates, and one ciphertext under the aggregated key"""

    def __init__(self):
        self.r = [0x1234567 + 977 * i for i in range(MEMBERS)]
        self.x = [0x7654321 + 313 * i for i in range(MEMBERS)]
        self.t = 0xabcdef12345
        self.X = [o.g1_mul(o.G1_GEN, x) for x in self.x]
        self.R = [o.g2_mul(o.G2_GEN, (-r) % o.R) for r in self.r]
        self.A = [o.pair([X], [o.G2_GEN]) for X in self.X]
        self.H = o.hash_to_g1(STRING, agka09.DST_BYTES_G1)
        self.sigma = [o.g1_add(X, o.g1_mul(self.H, r)) for X, r in zip(self.X, self.r)]
        self.aggR, self.aggA, self.agg_sigma = None, o.F12_ONE, None
        for R, A, s in zip(self.R, self.A, self.sigma):
            self.aggR, self.aggA, self.agg_sigma = o.g2_add(self.aggR, R), o.f12_mul(self.aggA, A), o.g1_add(self.agg_sigma, s)
        self.m = o.f12_pow(self.A[0], 0x5eed)                          # a plaintext in GT
        self.c1, self.c2 = o.g2_mul(o.G2_GEN, self.t), o.g2_mul(self.aggR, self.t)
        self.c3 = o.f12_mul(self.m, o.f12_pow(self.aggA, self.t))

    def rows(self, pts, to_bytes):
        return np.stack([arr(to_bytes(p)) for p in pts])


@pytest.fixture(scope="module")
def ref():
    return Asbb()


def test_keygen_and_sign_are_the_references(eng, ref):
    R, A, X = agka09.keygen_batch(eng, ref.r, ref.x)
    assert R.tobytes() == ref.rows(ref.R, o.g2_to_bytes).tobytes() and X.tobytes() == ref.rows(ref.X, o.g1_to_bytes).tobytes()
    assert A.shape == (MEMBERS, 384) and A.tobytes() == ref.rows(ref.A, o.gt_to_bytes).tobytes()
    sig = agka09.sign_batch(eng, ref.r, X, strings=[STRING] * MEMBERS)                     # a key per item
    assert sig.shape == (MEMBERS, 64) and sig.tobytes() == ref.rows(ref.sigma, o.g1_to_bytes).tobytes()
    one = agka09.sign_batch(eng, [ref.r[1]], X[1], strings=[STRING, b"another string"])     # one key for the batch
    assert one[0].tobytes() == sig[1].tobytes() and one[1].tobytes() != sig[1].tobytes()
    assert agka09.hash_strings(eng, [STRING])[0].tobytes() == o.g1_to_bytes(ref.H)
    assert (agka09.verify_each(eng, R, A, sig, strings=[STRING] * MEMBERS) == 1).all()
    assert agka09.verify_each(eng, R[1], A[1], sig, strings=[STRING] * MEMBERS).tolist() == [0, 1, 0]      # one key for the batch
    g1, g2 = agka09.public_params(eng)
    assert g1.tobytes() == o.g1_to_bytes(o.G1_GEN) and g2.tobytes() == o.g2_to_bytes(o.G2_GEN)


def test_verify_each_takes_the_references_pairs_in_the_references_order(oracle, ref):
    """Verify (asbb.go:123-146): e(sigma, g2), then e(H(s), R), their product, Equal against A"""
    eng = MemberStandIn(oracle)
    calls = recorded(eng, ["multi_pair", "gt_equal", "pair_batch"])
    R, A, sig = ref.rows(ref.R, o.g2_to_bytes), ref.rows(ref.A, o.gt_to_bytes), ref.rows(ref.sigma, o.g1_to_bytes)
    assert (agka09.verify_each(eng, R, A, sig, strings=[STRING] * MEMBERS) == 1).all()
    assert [c[0] for c in calls] == ["multi_pair", "gt_equal"]
    P, Q, seg = calls[0][1]
    H, G2 = o.g1_to_bytes(ref.H), o.g2_to_bytes(o.G2_GEN)
    assert np.asarray(P).tobytes() == b"".join(sig[i].tobytes() + H for i in range(MEMBERS))
    assert np.asarray(Q).tobytes() == b"".join(G2 + R[i].tobytes() for i in range(MEMBERS))
    assert [int(v) for v in seg] == [0, 2, 4, 6]
    left, right = calls[1][1]
    assert np.asarray(right).tobytes() == A.tobytes()
    want = [o.f12_mul(o.pair([s], [o.G2_GEN]), o.pair([ref.H], [r])) for s, r in zip(ref.sigma[:1], ref.R[:1])]
    assert np.asarray(left).reshape(-1, 384)[0].tobytes() == o.gt_to_bytes(want[0]) == o.gt_to_bytes(ref.A[0])


def test_key_homomorphism_with_three_members(eng, ref):
    """asbb.go:21-30: the aggregated signature on one string verifies under the aggregated key, and decrypts what was encrypted under it"""
    R, A, sig = ref.rows(ref.R, o.g2_to_bytes), ref.rows(ref.A, o.gt_to_bytes), ref.rows(ref.sigma, o.g1_to_bytes)
    aR, aA = agka09.aggregate_public_keys(eng, R, A, [0, MEMBERS])
    asig = agka09.aggregate_signatures(eng, sig, [0, MEMBERS])
    assert aR.shape == (1, 128) and aR.tobytes() == o.g2_to_bytes(ref.aggR) and aA.tobytes() == o.gt_to_bytes(ref.aggA)
    assert asig.shape == (1, 64) and asig.tobytes() == o.g1_to_bytes(ref.agg_sigma)
    assert agka09.verify_each(eng, aR, aA, asig, strings=[STRING]).tolist() == [1]
    assert agka09.verify_each(eng, aR, aA, sig[:1], strings=[STRING]).tolist() == [0]       # a member's own signature is none under it
    m = arr(o.gt_to_bytes(ref.m))
    c1, c2, c3 = agka09.encrypt_batch(eng, aR, aA, m, [ref.t])
    assert c1.tobytes() == o.g2_to_bytes(ref.c1) and c2.tobytes() == o.g2_to_bytes(ref.c2) and c3.tobytes() == o.gt_to_bytes(ref.c3)
    assert agka09.decrypt_batch(eng, c1, c2, c3, asig, strings=[STRING]).tobytes() == m.tobytes()
    assert agka09.decrypt_batch(eng, c1, c2, c3, sig[0], strings=[STRING]).tobytes() != m.tobytes()
    # two groups in one call, and the seeded form: ONE draw of n scalars
    two_R, two_A = agka09.aggregate_public_keys(eng, R, A, [0, 1, MEMBERS])
    assert two_R[0].tobytes() == R[0].tobytes() and two_A[0].tobytes() == A[0].tobytes()
    assert two_R[1].tobytes() == o.g2_to_bytes(o.g2_add(ref.R[1], ref.R[2]))
    rng = Randomness(eng, SEED)
    s1, s2, s3 = agka09.encrypt_batch_seeded(eng, aR, aA, np.stack([m, m]), rng)
    t = eng.fr_random(SEED, 2, stream=0)
    e1, e2, e3 = agka09.encrypt_batch(eng, aR, aA, np.stack([m, m]), t)
    assert rng.next_stream == 1 and (s1.tobytes(), s2.tobytes(), s3.tobytes()) == (e1.tobytes(), e2.tobytes(), e3.tobytes())
    assert s3[0].tobytes() != s3[1].tobytes()
    assert agka09.decrypt_batch(eng, s1, s2, s3, asig, strings=[STRING]).tobytes() == np.stack([m, m]).tobytes()


def test_validation_masks_zero_rows_and_what_enters_the_sums(oracle, ref):
    """group 0: three honest keys; group 1: an R off the subgroup; group 2: an A that is cyclotomic but not of order r; group 3: a
    non-canonical A beside an honest key.  The rejected elements reach g2_sum_segments / gt_prod as infinity / one."""
    eng = MemberStandIn(oracle)
    g2c, gtc = mc.g2_cases(), mc.gt_cases()
    R, A = ref.rows(ref.R, o.g2_to_bytes), ref.rows(ref.A, o.gt_to_bytes)
    bad_R, easy_A, big_A = g2c.data[g2c.of("off_subgroup")[0]], gtc.data[gtc.of("easy_part_only")[0]], gtc.data[gtc.of("coordinate_max")[0]]
    Rs = np.stack([R[0], R[1], R[2], bad_R, R[1], R[2], R[0], R[1]])
    As = np.stack([A[0], A[1], A[2], A[0], A[1], easy_A, big_A, A[1]])
    seg = [0, 3, 5, 6, 8]
    calls = recorded(eng, ["g2_sum_segments", "gt_prod"])
    aR, aA, ok, mask = agka09.aggregate_public_keys(eng, Rs, As, seg, validate=True)
    assert mask.dtype == np.uint8 and mask.tolist() == [1, 1, 1, 0, 1, 0, 0, 1] and ok.tolist() == [1, 0, 0, 0]
    assert aR[0].tobytes() == o.g2_to_bytes(ref.aggR) and aA[0].tobytes() == o.gt_to_bytes(ref.aggA)
    assert not aR[1:].any() and not aA[1:].any()
    summed, multiplied = np.asarray(calls[0][1][0]).reshape(-1, 128), np.asarray(calls[1][1][0]).reshape(-1, 384)
    for i, m in enumerate(mask):
        assert summed[i].tobytes() == (Rs[i].tobytes() if m else bytes(128)), i
        assert multiplied[i].tobytes() == (As[i].tobytes() if m else _plan.GT_ONE.tobytes()), i
    # without validation the same call sums whatever it is given: the aggregator without a defence
    uR, uA = agka09.aggregate_public_keys(eng, Rs, As, seg)
    assert uR[0].tobytes() == aR[0].tobytes() and uR[1].any() and uR[1].tobytes() != o.g2_to_bytes(ref.R[1])
    # signatures: one off the curve
    g1c = mc.g1_cases()
    sig = ref.rows(ref.sigma, o.g1_to_bytes)
    off = g1c.data[g1c.of("y_plus_one")[0]]
    sigs = np.stack([sig[0], sig[1], sig[2], sig[0], off])
    calls = recorded(eng, ["g1_sum_segments"])
    agg, sig_ok, sig_mask = agka09.aggregate_signatures(eng, sigs, [0, 3, 5], validate=True)
    assert sig_mask.tolist() == [1, 1, 1, 1, 0] and sig_ok.tolist() == [1, 0]
    assert agg[0].tobytes() == o.g1_to_bytes(ref.agg_sigma) and not agg[1].any()
    assert np.asarray(calls[0][1][0]).reshape(-1, 64)[4].tobytes() == bytes(64)
    # verify_each: a signature off the curve gets 0 and reaches the pairing as infinity
    calls = recorded(eng, ["multi_pair"])
    got = agka09.verify_each(eng, R[0], A[0], np.stack([sig[0], off]), strings=[STRING] * 2, validate=True)
    assert got.tolist() == [1, 0] and np.asarray(calls[0][1][0]).reshape(-1, 64)[2].tobytes() == bytes(64)
    # on CPU tensors through the engine's tensor behaviour
    import torch
    tR, tA = tensors(Rs, As)
    out = agka09.aggregate_public_keys(TensorEngine(eng), tR, tA, seg, validate=True)
    assert all(isinstance(v, torch.Tensor) for v in out)
    assert [v.numpy().tobytes() for v in out] == [aR.tobytes(), aA.tobytes(), ok.tobytes(), mask.tobytes()]


def test_an_empty_group_raises(eng, ref):
    R, A, sig = ref.rows(ref.R, o.g2_to_bytes), ref.rows(ref.A, o.gt_to_bytes), ref.rows(ref.sigma, o.g1_to_bytes)
    for seg in ([0, 0, 3], [0, 3, 3], [0]):
        with pytest.raises(ValueError, match="public keys"):
            agka09.aggregate_public_keys(eng, R, A, seg)
        with pytest.raises(ValueError, match="signatures"):
            agka09.aggregate_signatures(eng, sig, seg, validate=True)
    with pytest.raises(ValueError, match="public keys"):
        agka09.aggregate_public_keys(eng, R[:0], A[:0], [0, 0])
    with pytest.raises(ValueError):
        agka09.aggregate_public_keys(eng, R, A[:2], [0, 3])


def test_verify_batch_equals_verify_each(eng, oracle, ref):
    n = 5
    strings = [b"string %d" % i for i in range(n)]
    R, A, X = (v[0] for v in agka09.keygen_batch(eng, ref.r[:1], ref.x[:1]))
    sig = agka09.sign_batch(eng, ref.r[:1], X, strings=strings)
    hashed = agka09.hash_strings(eng, strings)
    for forged in ([], [3]):
        s = np.array(sig, copy=True)
        for i in forged:
            s[i] = sig[(i + 1) % n]
        want = agka09.verify_each(eng, R, A, s, strings=strings)
        assert want.tolist() == [0 if i in forged else 1 for i in range(n)]
        for group in (1, 2, 5, 1024):
            got = agka09.verify_batch(eng, R, A, s, Randomness(eng, SEED), hashed=hashed, group=group)
            assert got.dtype == np.uint8 and got.tolist() == want.tolist(), (forged, group)
    e = MemberStandIn(oracle)
    calls = recorded(e, ["multi_pair"])
    assert (agka09.verify_batch(e, R, A, sig, Randomness(e, SEED), strings=strings, group=2) == 1).all() and not calls      # no per-item pairing
    # S + D and S - D on ONE string: both invalid, every unweighted sum unchanged
    D = arr(o.g1_to_bytes(o.g1_mul(o.G1_GEN, 99)))
    two = agka09.sign_batch(eng, ref.r[:1], X, strings=[STRING, STRING])
    pair = np.stack([eng.g1_add(two[0], D)[0], eng.g1_sub(two[1], D)[0]])
    assert agka09.verify_each(eng, R, A, pair, strings=[STRING] * 2).tolist() == [0, 0]
    ones = np.tile(arr((1).to_bytes(32, "little")), (2, 1))
    assert agka09.verify_batch(eng, R, A, pair, ones, strings=[STRING] * 2, group=2).tolist() == [1, 1]      # weights all 1: the pair passes ...
    right = eng.gt_exp(A, np.frombuffer((2).to_bytes(32, "little"), dtype=np.uint8))
    left = agka09.group_values(eng, R, pair, agka09.hash_strings(eng, [STRING] * 2), ones.reshape(-1), np.array([0, 2], dtype=np.uint64))
    assert np.asarray(left).tobytes() == np.asarray(right).tobytes()                                    # ... because the group equation holds
    assert agka09.verify_batch(eng, R, A, pair, ones, strings=[STRING] * 2, group=1).tolist() == [0, 0]      # (alone, each fails)
    assert agka09.verify_batch(eng, R, A, pair, Randomness(eng, SEED), strings=[STRING] * 2, group=2).tolist() == [0, 0]
    rho = Randomness(eng, SEED).scalars(pair, 2).reshape(-1)
    assert np.asarray(agka09.group_values(eng, R, pair, agka09.hash_strings(eng, [STRING] * 2), rho, np.array([0, 2], dtype=np.uint64))).tobytes() != \
        np.asarray(eng.gt_exp(A, eng.fr_sum_segments(rho, [0, 2]))).tobytes()
    with pytest.raises(ValueError, match="non-zero"):
        agka09.verify_batch(eng, R, A, pair, np.zeros((2, 32), dtype=np.uint8), strings=[STRING] * 2)
    assert agka09.verify_batch(eng, R, A, sig[:0], Randomness(eng, SEED), strings=[]).shape == (0,)
