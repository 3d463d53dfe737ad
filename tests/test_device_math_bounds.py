"""CPU verification of the DEVICE arithmetic: csrc/fe29.hip.hpp .. pairing29.hip.hpp compiled for the host with
-DGPBC_BOUNDS (tools/bounds_check.cpp).  In that build every field element carries data-independent magnitude
bounds and every Montgomery product aborts if its int64 column accumulators could overflow for ANY input, so a
run that finishes is a proof of overflow-freedom for the straight-line code paths it exercised; the values it
computes are the exact values the GPU computes, and are compared with the oracle bit for bit.
(Verification harness only: the product has no CPU fallback and never loads this library.)"""
import ctypes
import os

import numpy as np

import bn254_py as o
from conftest import ROOT, cat, load_golden
from bounds_harness import hc  # noqa: F401  (the fixture)



def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_pairing_golden_under_bounds(hc):
    g = load_golden("pairing.json")["cases"][:12]          # includes the infinity cases
    P, Q = cat([c["P"] for c in g]).copy(), cat([c["Q"] for c in g]).copy()
    out = np.zeros((len(g), 384), dtype=np.uint8)
    hc.hc_pair(vp(P), vp(Q), ctypes.c_size_t(len(g)), vp(out))
    for i, c in enumerate(g):
        assert out[i].tobytes().hex() == c["GT"], c["note"]


def test_scalar_mul_golden_under_bounds(hc):
    for name, fn, w in (("g1_scalar_mul.json", hc.hc_g1_mul, 64), ("g2_scalar_mul.json", hc.hc_g2_mul, 128)):
        g = load_golden(name)["cases"]
        B, K = cat([c["base"] for c in g]).copy(), cat([c["scalar"] for c in g]).copy()
        out = np.zeros((len(g), w), dtype=np.uint8)
        fn(vp(B), vp(K), ctypes.c_size_t(len(g)), vp(out))
        for i, c in enumerate(g):
            assert out[i].tobytes().hex() == c["out"], (name, i, c["note"])


def test_field_and_gt_ops_under_bounds(hc, oracle):
    rng = np.random.default_rng(29)
    n = 512
    vals = [int.from_bytes(rng.bytes(32), "little") % o.P for _ in range(2 * n)]
    vals[0], vals[1], vals[n], vals[n + 1] = 0, o.P - 1, o.P - 1, o.P - 1
    a = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals[:n]), dtype=np.uint8).copy()
    b = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals[n:]), dtype=np.uint8).copy()
    out = np.zeros((n, 32), dtype=np.uint8)
    hc.hc_fp_mul(vp(a), vp(b), ctypes.c_size_t(n), vp(out))
    assert (out == oracle.fp_mul(a, b)).all()
    g = load_golden("gt_ops.json")["binary"]
    A, B = cat([c["a"] for c in g]).copy(), cat([c["b"] for c in g]).copy()
    m = np.zeros((len(g), 384), dtype=np.uint8)
    hc.hc_gt_mul(vp(A), vp(B), ctypes.c_size_t(len(g)), vp(m))
    inv = np.zeros((len(g), 384), dtype=np.uint8)
    hc.hc_gt_inv(vp(A), ctypes.c_size_t(len(g)), vp(inv))
    sq = np.zeros((len(g), 384), dtype=np.uint8)
    hc.hc_gt_sqr(vp(A), ctypes.c_size_t(len(g)), vp(sq), ctypes.c_int(0))
    cs = np.zeros((len(g), 384), dtype=np.uint8)
    hc.hc_gt_sqr(vp(A), ctypes.c_size_t(len(g)), vp(cs), ctypes.c_int(1))
    dv = np.zeros((len(g), 384), dtype=np.uint8)
    hc.hc_gt_div(vp(A), vp(B), ctypes.c_size_t(len(g)), vp(dv))            # pairing values: norm one, the conjugate path of k_gt_binary
    for i, c in enumerate(g):
        assert m[i].tobytes().hex() == c["mul"] and inv[i].tobytes().hex() == c["inv_a"] and dv[i].tobytes().hex() == c["div"]
    assert (sq == oracle.gt_mul(A, A)).all() and (cs == sq).all()
    # ... and divisors of norm other than one (random Fp12 elements): the general path
    rnd = np.frombuffer(b"".join((int.from_bytes(rng.bytes(32), "little") % o.P).to_bytes(32, "little") for _ in range(12 * 4)), dtype=np.uint8)
    Bm = oracle.fp_mul(rnd, np.frombuffer(b"".join((pow(2, 512, o.P)).to_bytes(32, "little") for _ in range(48)), dtype=np.uint8)).reshape(4, 384).copy()   # to Montgomery form
    dv2 = np.zeros((4, 384), dtype=np.uint8)
    A4 = A.reshape(-1, 384)[:4].copy()
    hc.hc_gt_div(vp(A4), vp(Bm), ctypes.c_size_t(4), vp(dv2))
    assert (dv2 == oracle.gt_div(A4, Bm)).all()


def test_bound_margins(hc):
    """The worst case over everything run above stays inside int64 columns / int32 limbs."""
    st = np.zeros(7)
    hc.hc_stats(vp(st))
    assert 0 < st[0] < 2.0**63 and st[1] < 2.0**31 and st[2] < 128 and st[3] > 1e5


def test_lane_pair_forms_under_bounds(hc, oracle):
    """tower29_pair.hip.hpp / pairing29_pair.hip.hpp: one Fp12 value per lane pair (two host threads + rendezvous stand in for
    the DPP swap).  Every pair-form operation and the full pair-form pairing must match the oracle bit for bit."""
    n = 3
    g1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
    g2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
    k = np.frombuffer(b"".join(o.scalar_to_bytes(o.bench_scalar("P", 40 + i)) for i in range(n)), dtype=np.uint8).copy()
    P, Q = oracle.g1_scalar_mul(g1, k), oracle.g2_scalar_mul(g2, k)
    ref = oracle.pair_batch(P, Q)
    A, B = ref.copy(), np.roll(ref, 1, axis=0).copy()
    outs = [np.zeros((n, 384), dtype=np.uint8) for _ in range(5)]
    hc.hc_gt_pair_ops(vp(A), vp(B), ctypes.c_size_t(n), *[vp(x) for x in outs])
    assert (outs[0] == oracle.gt_mul(A, B)).all()
    assert (outs[1] == oracle.gt_mul(A, A)).all() and (outs[2] == outs[1]).all()
    assert (outs[3] == oracle.gt_inverse(A)).all()
    frob = np.frombuffer(b"".join(o.gt_to_bytes(o.f12_frobenius(o.gt_from_bytes(A[i].tobytes()))) for i in range(n)),
                         dtype=np.uint8).reshape(n, 384)
    assert (outs[4] == frob).all()
    f = np.zeros((n, 384), dtype=np.uint8)
    hc.hc_pair_lanes(vp(P), vp(Q), ctypes.c_size_t(n), vp(f), ctypes.c_int(0))
    assert (oracle.final_exp(f) == ref).all()
    gt = np.zeros((n, 384), dtype=np.uint8)
    hc.hc_pair_lanes(vp(P), vp(Q), ctypes.c_size_t(n), vp(gt), ctypes.c_int(1))
    assert (gt == ref).all()


def test_multi_pairing_flows_under_bounds(hc, oracle):
    """The two multi-pairing accumulators as the kernels run them: shared squarings over the scaled lines of a chunk
    (k_miller_accumulate_chunks) and the fixed-Q form — raw line coefficients of every Q_i, evaluated at P_i by two
    Fp x Fp2 products right before the sparse multiplication (k_q_lines + k_miller_accumulate_fixed_q).  Both must be
    overflow-free for any input and give the oracle's product of pairings."""
    n = 5
    g1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
    g2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
    kp = np.frombuffer(b"".join(o.scalar_to_bytes(o.bench_scalar("P", 70 + i)) for i in range(n)), dtype=np.uint8).copy()
    kq = np.frombuffer(b"".join(o.scalar_to_bytes(o.bench_scalar("Q", 70 + i)) for i in range(n)), dtype=np.uint8).copy()
    P, Q = oracle.g1_scalar_mul(g1, kp), oracle.g2_scalar_mul(g2, kq)
    want = oracle.multi_pair(P, Q, np.array([0, n], dtype=np.uint64))
    f = np.zeros((1, 384), dtype=np.uint8)
    hc.hc_pair_lanes_multi(vp(P), vp(Q), ctypes.c_size_t(n), vp(f))
    assert (oracle.final_exp(f) == want).all()
    f2 = np.zeros((1, 384), dtype=np.uint8)
    hc.hc_pair_fixed_q(vp(P), vp(Q), ctypes.c_size_t(n), vp(f2), ctypes.c_int(0))
    assert (oracle.final_exp(f2) == want).all()
    gt = np.zeros((1, 384), dtype=np.uint8)
    hc.hc_pair_fixed_q(vp(P), vp(Q), ctypes.c_size_t(n), vp(gt), ctypes.c_int(1))
    assert (gt == want).all()


def test_wnaf_digits_of_u():
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "gopairingbasedcryptography_amd", "csrc", "bn254_constants.hip.hpp")).read()
    digits = [int(x) for x in re.search(r"#define GPBC_U_WNAF4 \{([^}]*)\}", text).group(1).split(",")]
    assert sum(d << i for i, d in enumerate(digits)) == o.U and all(d == 0 or (d % 2 and abs(d) < 8) for d in digits)
    # the device chain: digits over the dictionary {x^3, x^15, x^75}
    chain = [int(x) for x in re.search(r"#define GPBC_U_CHAIN \{([^}]*)\}", text).group(1).split(",")]
    assert sum(d << i for i, d in enumerate(chain)) == o.U and all(abs(d) in (0, 3, 15, 75) for d in chain) and chain[-1] > 0
    assert len(chain) == int(re.search(r"#define GPBC_U_CHAIN_LEN (\d+)", text).group(1))


def test_glv_split_identity(hc):
    """k == k1 + k2*lambda (mod r) with |k1|,|k2| < 2^130 for edge and random 256-bit scalars (curve29.hip.hpp glv_split)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_constants as gc
    lam = gc.glv_constants()[0]
    rng = np.random.default_rng(5)
    ks = [0, 1, 2, o.R - 1, o.R, o.R + 5, (1 << 256) - 1, 1 << 255, lam, lam + 1, o.R - lam] + \
         [int.from_bytes(rng.bytes(32), "little") for _ in range(300)]
    K = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in ks), dtype=np.uint8).copy()
    out = np.zeros((len(ks), 12), dtype=np.uint32)
    hc.hc_glv_split(vp(K), ctypes.c_size_t(len(ks)), vp(out))
    for k, row in zip(ks, out):
        k1 = sum(int(row[i]) << (32 * i) for i in range(5)) * (-1 if row[10] else 1)
        k2 = sum(int(row[5 + i]) << (32 * i) for i in range(5)) * (-1 if row[11] else 1)
        assert (k1 + k2 * lam - k) % o.R == 0 and abs(k1).bit_length() <= 130 and abs(k2).bit_length() <= 130


def test_gt_exp_pair_under_bounds(hc):
    """k_gt_exp's lane-pair windowed exponentiation (generic squarings): pairing values and random Fp12 elements, edge
    exponents 0, 1, 15, 16, r-1, 2^256-1."""
    import random
    random.seed(3)
    e = o.pair([o.G1_GEN], [o.G2_GEN])
    rnd = lambda: tuple(tuple((random.randrange(o.P), random.randrange(o.P)) for _ in range(3)) for _ in range(2))
    A, K, exp = [], [], []
    for x, ks in ((e, [0, 1, 2, 15, 16, o.R - 1, (1 << 256) - 1, random.randrange(1 << 256)]), (rnd(), [3, random.randrange(1 << 256)])):
        for k in ks:
            A.append(o.gt_to_bytes(x)); K.append(k.to_bytes(32, "little")); exp.append(o.gt_to_bytes(o.f12_pow(x, k)))
    a = np.frombuffer(b"".join(A), dtype=np.uint8).copy()
    k = np.frombuffer(b"".join(K), dtype=np.uint8).copy()
    out = np.zeros(len(A) * 384, dtype=np.uint8)
    hc.hc_gt_exp_pair(vp(a), vp(k), ctypes.c_size_t(len(A)), vp(out))
    assert out.tobytes() == b"".join(exp)


def test_safegcd_inversion_matches_fermat_and_oracle(hc):
    """fe_inv (Bernstein-Yang divsteps, 600 constant-time steps on 30-bit limbs) against the Fermat power of the same
    header and against Python's pow: edge values (0 -> 0, 1, p-1, powers of two) and 2000 random elements."""
    import random
    random.seed(7)
    vals = [0, 1, 2, o.P - 1, o.P - 2, (o.P - 1) // 2, 3, 1 << 253] + [1 << k for k in range(0, 254, 7)] + [random.randrange(o.P) for _ in range(2000)]
    a = np.frombuffer(b"".join(o.fp_to_mont_bytes(v) for v in vals), dtype=np.uint8).copy()
    o1, o2 = np.zeros(len(vals) * 32, dtype=np.uint8), np.zeros(len(vals) * 32, dtype=np.uint8)
    hc.hc_fp_inv(vp(a), ctypes.c_size_t(len(vals)), vp(o1), vp(o2))
    exp = b"".join(o.fp_to_mont_bytes(pow(v, o.P - 2, o.P)) for v in vals)
    assert o1.tobytes() == exp and o2.tobytes() == exp


def test_divstep_legendre_symbol(hc):
    """fe_legendre (posdivsteps with the reciprocity rules, the is_square of hash to curve) against Euler's criterion: edge values,
    powers of two, squares and non-squares; 0 (not determined) is allowed only for a = 0 or beyond the 960-step budget, and must
    be rare."""
    import random
    random.seed(77)
    vals = [0, 1, 2, 3, 4, 5, o.P - 1, o.P - 2, (o.P - 1) // 2, (o.P + 1) // 2, 1 << 253] + [1 << k for k in range(0, 254, 5)]
    vals += [random.randrange(o.P) for _ in range(4000)] + [pow(random.randrange(1, o.P), 2, o.P) for _ in range(500)]
    a = np.frombuffer(b"".join(o.fp_to_mont_bytes(v) for v in vals), dtype=np.uint8).copy()
    out = np.zeros(len(vals), dtype=np.int8)
    hc.hc_fp_legendre(vp(a), ctypes.c_size_t(len(vals)), vp(out))
    undecided = 0
    for v, j in zip(vals, out):
        e = pow(v, (o.P - 1) // 2, o.P)
        e = -1 if e == o.P - 1 else e
        if j == 0:
            undecided += v != 0
        else:
            assert int(j) == e, (v, int(j), e)
    assert out[0] == 0 and undecided == 0


def test_fixed_base_msm_under_bounds(hc):
    """The table-build and 32-additions-per-term loop of k_g1_fb_build / k_g1_fb_msm on the host under the bounds
    harness (a subset of table rows is built; scalars only use digits of that subset), against the oracle."""
    import random
    random.seed(12)
    allowed = [0, 1, 2, 3, 4, 41, 78, 115, 152, 189, 226]
    def scalar():
        return sum((random.randrange(256) if w % 5 == 0 else random.choice(allowed)) << (8 * w) for w in range(32))
    nbase, n_msm = 3, 4
    bases = [o.g1_mul(o.G1_GEN, 5 + 11 * j) for j in range(nbase)]
    bases[1] = None                                                     # a base at infinity contributes nothing
    ks = [[scalar() for _ in range(nbase)] for _ in range(n_msm)]
    ks[0][0] = 0
    B = np.frombuffer(b"".join(o.g1_to_bytes(b) for b in bases), dtype=np.uint8).copy()
    K = np.frombuffer(b"".join(k.to_bytes(32, "little") for row in ks for k in row), dtype=np.uint8).copy()
    out = np.zeros(n_msm * 64, dtype=np.uint8)
    hc.hc_g1_fb_msm(vp(B), ctypes.c_size_t(nbase), vp(K), ctypes.c_size_t(n_msm), vp(out))
    for m in range(n_msm):
        acc = None
        for j in range(nbase):
            acc = o.g1_add(acc, o.g1_mul(bases[j], ks[m][j] % o.R) if bases[j] else None)
        assert out[64 * m:64 * m + 64].tobytes() == o.g1_to_bytes(acc), m


def test_gls_split_identity_and_size(hc):
    """gls_split: k = k0 + k1 mu + k2 mu^2 + k3 mu^3 (mod r), mu = 6u^2 (psi's eigenvalue on G2), |k_i| < 2^66, for edge
    scalars (0, 1, r-1, r, 2^256-1, mu, mu^2 ...) and 20000 random ones; and psi(Q) = [mu]Q in the oracle."""
    import random
    random.seed(66)
    mu = 6 * o.U * o.U % o.R
    Q = o.g2_mul(o.G2_GEN, 987654321)
    assert o.g2_frobenius(Q) == o.g2_mul(Q, mu)
    ks = [0, 1, 2, o.R - 1, o.R, o.R + 1, (1 << 256) - 1, mu, mu - 1, mu * mu % o.R, pow(mu, 3, o.R), o.R // 2, 1 << 255]
    ks += [random.randrange(1 << 256) for _ in range(20000)]
    K = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in ks), dtype=np.uint8).copy()
    out = np.zeros(16 * len(ks), dtype=np.uint32)
    hc.hc_gls_split(vp(K), ctypes.c_size_t(len(ks)), vp(out))
    out = out.reshape(len(ks), 4, 4)
    for t, k in enumerate(ks):
        acc = 0
        for i in range(4):
            mag = int(out[t, i, 0]) | int(out[t, i, 1]) << 32 | int(out[t, i, 2]) << 64
            assert mag < 1 << 66
            acc += (-mag if out[t, i, 3] else mag) * pow(mu, i, o.R)
        assert acc % o.R == k % o.R, k


def test_g2_glv_loop_still_agrees(hc):
    """The two-dimensional GLV loop instantiated for Fp2 (kept for comparison; the G2 kernels use the GLS loop) on the
    golden scalars."""
    g = load_golden("g2_scalar_mul.json")["cases"]
    B, K = cat([c["base"] for c in g]).copy(), cat([c["scalar"] for c in g]).copy()
    out = np.zeros((len(g), 128), dtype=np.uint8)
    hc.hc_g2_mul_glv(vp(B), vp(K), ctypes.c_size_t(len(g)), vp(out))
    for i, c in enumerate(g):
        assert out[i].tobytes().hex() == c["out"], i


def test_bucket_msm_under_bounds(hc, oracle):
    """csrc/msm29.hip.hpp — the per-lane pieces of the bucket (Pippenger) multi-scalar multiplication in the order the kernels of
    csrc/gpbc_msm.hip run them, G1 and G2, two window sizes: overflow-free for any input and equal to the oracle's
    sum of scalar multiplications.  Inputs include a point at infinity, zero / tiny / full-width scalars and a repeated base
    (an addition that must fall back to a doubling)."""
    n = 41
    g1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
    g2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
    kb = np.frombuffer(b"".join(o.scalar_to_bytes(o.bench_scalar("P", 300 + i)) for i in range(n)), dtype=np.uint8).copy()
    rng = np.random.default_rng(77)
    K = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    K[0] = 0; K[1] = 0; K[1, 0] = 1; K[2] = 255; K[3, 16:] = 0; K[4, 2:] = 0
    for name, gen, mul, summ, w in (("g1", g1, oracle.g1_scalar_mul, oracle.g1_sum, 64), ("g2", g2, oracle.g2_scalar_mul, oracle.g2_sum, 128)):
        B = np.asarray(mul(gen, kb)).reshape(n, w).copy()
        B[7] = 0                                                     # point at infinity
        B[9] = B[8]; K[9] = K[8]                                     # same base, same digits: P + P inside a bucket
        want = np.asarray(summ(mul(B.reshape(-1), K.reshape(-1)))).reshape(-1)
        for c in (8, 5):
            out = np.zeros(w, dtype=np.uint8)
            hc.hc_msm(ctypes.c_int(1 if name == "g2" else 0), vp(B), vp(K), ctypes.c_size_t(n), ctypes.c_int(c), vp(out))
            assert (out == want).all(), (name, c)


def test_executed_mad_counts_file_is_current(hc):
    """profiles/executed_mads.json (what bench.py's `executed_mad_*` fields are computed from) equals the harness's count of the
    MADs the device code issues per pairing / scalar multiplication (tests/executed_mads.py regenerates it)."""
    import json
    import executed_mads
    got = executed_mads.count(hc, n=4)                                       # the same four inputs the file was made from
    doc = json.load(open(os.path.join(ROOT, "profiles", "executed_mads.json")))
    for unit, want in doc["mads_per_unit"].items():
        assert abs(got[unit] - want) <= 1, (unit, got[unit], want)
    # the device does 81 limb products where SURVEY's nominal CIOS has 64, and lazy Fp2 products: more MADs than nominal for the pairing
    assert doc["mads_per_unit"]["pairing"] > doc["nominal_mac_per_unit"]["pairing"]


def test_wide_latency_form_under_bounds(hc, oracle):
    """csrc/wide29.hip.hpp: one pairing per wavefront, Fp12 values as F2 slots in LDS, the lanes of a wave working on the F2 products
    inside ONE pairing (the latency path of Pair / PairingCheck).  The host harness runs the lanes of every phase one after the
    other on interval-carrying slots: Miller value (through the oracle's final exponentiation) and the full pairing must match the
    oracle bit for bit, a point at infinity gives one, and no int64 column / int32 limb can overflow for any input."""
    n = 3
    g1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
    g2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
    k = np.frombuffer(b"".join(o.scalar_to_bytes(o.bench_scalar("wide", 7 + i)) for i in range(n)), dtype=np.uint8).copy()
    P, Q = oracle.g1_scalar_mul(g1, k), oracle.g2_scalar_mul(g2, k)
    P = np.ascontiguousarray(P); Q = np.ascontiguousarray(Q)
    ref = oracle.pair_batch(P, Q)
    f = np.zeros((n, 384), dtype=np.uint8)
    hc.hc_pair_wide(vp(P), vp(Q), ctypes.c_size_t(n), vp(f), ctypes.c_int(0))
    assert (oracle.final_exp(f) == ref).all()
    gt = np.zeros((n, 384), dtype=np.uint8)
    hc.hc_pair_wide(vp(P), vp(Q), ctypes.c_size_t(n), vp(gt), ctypes.c_int(1))
    assert (gt == ref).all()
    P0 = P.copy(); P0[1] = 0
    hc.hc_pair_wide(vp(P0), vp(Q), ctypes.c_size_t(n), vp(gt), ctypes.c_int(1))
    assert (gt == oracle.pair_batch(P0, Q)).all()
    # GT.Exp of the latency form (wide_exp256) on a pairing value and on Miller values (outside the cyclotomic subgroup): the chain of
    # general products z <- z z, z <- z x^d must hold its bounds for any exponent, the all-ones one included
    x = np.ascontiguousarray(np.concatenate([ref[:1], f[:2]]))
    ks = np.frombuffer(b"".join(e.to_bytes(32, "little") for e in ((1 << 256) - 1, o.bench_scalar("wide-exp", 0), 0)), dtype=np.uint8).copy()
    got = np.zeros((3, 384), dtype=np.uint8)
    hc.hc_gt_exp_wide(vp(x), vp(ks), ctypes.c_size_t(3), vp(got))
    assert (got == oracle.gt_exp(x, ks, threads=3)).all()
