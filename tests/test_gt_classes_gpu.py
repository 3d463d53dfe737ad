"""The GT entries on the device over every class of Fp12 element and every wavefront mix (tests/f12_cases.py): gt_exp in both forms,
gt_mul / gt_div / gt_inverse, final_exp in both forms, gt_multi_exp, GTFixedBase and gt_equal, byte for byte against the big-integer
expectations (f12_pow with the exponent unreduced, f12_inv with 1 / 0 = 0, final_exp_direct).

The kernels vote per wavefront — Granger-Scott squarings when every base is cyclotomic (32 elements per wavefront in k_gt_exp and
k_gt_multi_exp), the conjugate when every divisor has norm one (64 per wavefront in k_gt_binary) — so the layouts put ONE foreign
element at lane 0 of a wavefront, at its last lane and alone in the partial last wavefront, beside wavefronts that stay uniform.  The
foreigner that matters is `norm_one_only`: norm one, not cyclotomic."""
import numpy as np
import pytest

import bn254_py as o
import f12_cases as fc

pytestmark = pytest.mark.gpu

GT = fc.GT
ONE = fc.to_row(o.F12_ONE)
KNOBS = (0, 2048)                                                      # gpbc_set_latency_path: lane-pair kernels only / the default


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


@pytest.fixture(params=KNOBS)
def knob(request, eng):
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    _lib.check(lib.gpbc_set_latency_path(request.param))
    try:
        yield request.param
    finally:
        lib.gpbc_set_latency_path(2048)


def rows(idx):
    return np.ascontiguousarray(fc.corpus().rows[idx])


def bad_rows(got, want, idx):
    c = fc.corpus()
    return [c.describe(int(idx[j])) + " at %d" % j for j in np.nonzero((np.asarray(got).reshape(-1, GT) != want).any(1))[0]]


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_gt_exp_in_every_layout(eng, knob):
    """knob 0: k_gt_exp, 32 elements per wavefront under one vote; 2048: k_gt_exp_wide, an element per wavefront"""
    bad = []
    for t, (label, idx) in enumerate(fc.layouts()):
        ks = fc.exponents_for(idx, t)
        got = eng.gt_exp(rows(idx), fc.exponent_rows(ks).reshape(-1))
        bad += [label + ": " + b for b in bad_rows(got, fc.want_exp(idx, ks), idx)]
    assert not bad, bad[:8]
    idx, ks = fc.class_exponent_cases()                                 # and every class under every exponent, as one call
    assert not bad_rows(eng.gt_exp(cuda(rows(idx)), cuda(fc.exponent_rows(ks).reshape(-1))).cpu().numpy(), fc.want_exp(idx, ks), idx)


def test_gt_mul_div_inverse_with_every_layout_as_the_divisor(eng):
    """k_gt_binary: an element per lane, 64 divisors under one norm-one vote"""
    m = len(fc.corpus())
    bad = []
    for label, b in fc.layouts():
        a = (7 * np.arange(len(b)) + 3) % m
        xa, xb = rows(a), rows(b)
        for name, got, want in (("div", eng.gt_div(xa, xb), fc.want_div(a, b)), ("mul", eng.gt_mul(xa, xb), fc.want_mul(a, b)),
                                ("inverse", eng.gt_inverse(xb), fc.want_inverse(b))):
            bad += ["%s, %s: %s" % (name, label, r) for r in bad_rows(got, want, b)]
    assert not bad, bad[:8]


def test_final_exp_of_every_class_and_layout(eng, knob):
    """knob 0: k_final_exp (lane pairs); 2048: k_final_exp_wide for the layouts and the corpus.  Host arrays and CUDA tensors."""
    c = fc.corpus()
    every = np.arange(len(c))
    want = fc.want_final_exp(every)
    for i in every:
        if c.cls[i] in fc.EASY_PART_ONE:
            assert want[i].tobytes() == ONE.tobytes(), c.describe(i)
    cases = [("the corpus", every)] + fc.layouts() + [("the corpus tiled", np.resize(every, 2108))]       # 68 x 31: above 2 048 elements
    bad = []
    for label, idx in cases:
        w = want[idx]
        bad += ["host, %s: %s" % (label, r) for r in bad_rows(eng.final_exp(rows(idx)), w, idx)]
        bad += ["device, %s: %s" % (label, r) for r in bad_rows(eng.final_exp(cuda(rows(idx))).cpu().numpy(), w, idx)]
    assert not bad, bad[:8]


def test_gt_multi_exp_groups_next_to_each_other(eng):
    """32 segments of four factors are the 32 lane pairs of a wavefront: one of cyclotomic groups, one of cyclotomic groups with a
    norm_one_only group and the one-in-four groups among them, one of norm_one_only groups, then every class four at a time"""
    idx, ks, seg = fc.multi_exp_case(32)
    assert fc.R in ks and (1 << 256) - 1 in ks and len(seg) - 1 > 3 * 32
    want = fc.want_multi_exp(idx, ks, seg)
    x, k = rows(idx).reshape(-1), fc.exponent_rows(ks).reshape(-1)
    for got in (eng.gt_multi_exp(x, k, seg), eng.gt_multi_exp(cuda(x), cuda(k), seg).cpu().numpy()):
        bad = [s for s in range(len(seg) - 1) if np.asarray(got).reshape(-1, GT)[s].tobytes() != want[s].tobytes()]
        assert not bad, [(s, [fc.corpus().cls[i] for i in idx[seg[s]:seg[s + 1]]]) for s in bad[:8]]


def test_fixed_base_tables_of_bases_outside_gt(eng):
    """norm_one_only, cyclotomic_not_gt and -e(P, Q) beside a pairing value: the build squares generically whatever the base"""
    c = fc.corpus()
    bases = [c.of(cls)[0] for cls in ("pairing", "norm_one_only", "cyclotomic_not_gt", "minus_pairing")]
    ks = [fc.R - 1, fc.R, fc.R + 1, (1 << 256) - 1]
    fb = eng.GTFixedBase(rows(bases))
    try:
        for j, i in enumerate(bases):
            assert not bad_rows(fb.pow(ks, base=j), fc.want_exp([i] * len(ks), ks), [i] * len(ks))
        index = [[j, (j + 1) % len(bases)] for j in range(len(bases))]
        out, ok = fb.indexed(index, [[ks[j], ks[(j + 2) % 4]] for j in range(len(bases))])
        want = fc.rows_of(o.f12_mul(fc.power(bases[a], ks[j]), fc.power(bases[b], ks[(j + 2) % 4])) for j, (a, b) in enumerate(index))
        assert ok.all() and (out == want).all()
    finally:
        fb.close()


def test_gt_equal_and_is_one_on_every_class(eng):
    """x against x, conj(x), -x and one, compared as the bytes they are; only `one` is one"""
    c = fc.corpus()
    x = c.rows
    conj, neg = fc.rows_of(o.f12_conj(z) for z in c.val), fc.rows_of(fc.f12_neg(z) for z in c.val)
    for other in (x, conj, neg, np.tile(ONE, (len(c), 1))):
        want = [int(a.tobytes() == b.tobytes()) for a, b in zip(x, other)]
        assert eng.gt_equal(x, np.ascontiguousarray(other)).tolist() == want
        assert eng.gt_equal(cuda(x), cuda(other)).cpu().tolist() == want
    is_one = eng.gt_equal(x, ONE).tolist()
    assert is_one == [int(cls == "one") for cls in c.cls] and sum(is_one) == 1
    assert eng.gt_equal(conj, ONE).tolist() == is_one and eng.gt_equal(neg, ONE).tolist() == [int(cls == "minus_one") for cls in c.cls]
    # k_gt_is_one takes GT values only from a pairing product: e(P, Q) e(-P, Q) is one; e(P, Q), its square and e(-P, Q) are not
    g1, g2 = eng.generators()
    minus = np.frombuffer(o.g1_to_bytes(o.g1_neg(o.G1_GEN)), dtype=np.uint8)
    P, Q = np.concatenate([g1, minus, g1, g1, g1, minus]), np.tile(g2, 6)
    assert eng.pairing_check_batch(P, Q, [0, 2, 3, 5, 6]).tolist() == [True, False, False, False]
