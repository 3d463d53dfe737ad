"""Opening proofs over ragged batches on the MI355X (run with -m gpu): k_fr_poly_from_roots_segments, k_g1/g2_fb_openings and the mask through
bn254.fr_poly_from_roots_segments and bn254.FixedBase.openings, that is through the C entries of include/gpbc_bn254_openings.h in the host
form and the _dev form.  Everything is bit-exact.

  * nbase = 17 with batches of 16, 16, 1, 5, 0, 16 (one base per lane, 17 chunks, two levels of sums) and the corpus of
    tests/openings_cases.py on its own small tables (a repeated identity, residues, tau among the identities): against Python integers and
    the C oracle's scalar multiplications and sums — never against the code under test;
  * nbase = 257 with 8 full batches of 256 (four bases per lane, 65 chunks, two levels) against fr_poly_from_roots + fr_poly_quotients +
    FixedBase.msm in the same process: the route the fused kernel replaces, an independent device path;
  * G1, nbase = 300 with batches of 299 and 3: the instance of the staging that holds up to 1024 coefficients, the long batch against the
    same existing route, the short one against [q(tau)] g;
  * 24 calls with different segment tables in flight on a side stream: the _dev forms copy the host table before they return."""
import numpy as np
import pytest

import openings_cases as oc

pytestmark = pytest.mark.gpu
R = oc.R
GROUPS = pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def powers(eng, g2, nbase):
    """[tau^c] of the generator for c < nbase, from the engine's own generator multiplication on Python-integer powers"""
    mul = eng.g2_scalar_mul_base if g2 else eng.g1_scalar_mul_base
    return np.asarray(mul([pow(oc.TAU, c, R) for c in range(nbase)])).reshape(nbase, -1)


@pytest.fixture(scope="module")
def tables(eng):
    """{(g2, nbase): FixedBase over [tau^c]}, alive for the whole module; the small ones from the corpus' Python-integer bases"""
    t = {}
    for g2 in (False, True):
        t[g2, oc.NBASE[g2]] = eng.FixedBase(oc.bases(g2), g2=g2)
        t[g2, 17] = eng.FixedBase(to_dev(powers(eng, g2, 17)), g2=g2)
        t[g2, 257] = eng.FixedBase(powers(eng, g2, 257), g2=g2)
    t[False, 300] = eng.FixedBase(powers(eng, False, 300))
    yield t
    for table in t.values():
        table.close()


def both_forms(eng, table, ids, counts):
    """the host form and the _dev form of the two entries on one call: [(form, coeffs, points, ok)] as host arrays"""
    import torch
    K = oc.scalar_rows(ids)
    coeffs = eng.fr_poly_from_roots_segments(K, counts, table.nbase)
    pts, ok = table.openings(K, counts, coeffs=coeffs.reshape(-1))
    assert isinstance(pts, np.ndarray) and pts.dtype == np.uint8 and isinstance(ok, np.ndarray) and coeffs.shape == (len(counts), table.nbase, 32)
    dco = eng.fr_poly_from_roots_segments(to_dev(K), counts, table.nbase)
    dpts, dok = table.openings(to_dev(K), counts)                                         # the coefficients made inside
    assert dpts.is_cuda and dpts.dtype == torch.uint8 and dok.is_cuda and dco.is_cuda
    return [("host", coeffs, pts, ok), ("device", dco.cpu().numpy(), dpts.cpu().numpy(), dok.cpu().numpy())]


def at_tau(eng, g2, ids):
    """[q(tau)] g for every identity of ONE batch of distinct identities: a second statement of the opening, through the engine's
    generator multiplication"""
    f = oc.poly_from_roots([v % R for v in ids])
    vals = []
    for v in ids:
        q, rem = oc.quotient(f, v % R)
        assert rem == 0
        vals.append(sum(c * pow(oc.TAU, e, R) for e, c in enumerate(q)) % R)
    return np.asarray((eng.g2_scalar_mul_base if g2 else eng.g1_scalar_mul_base)(vals)).reshape(len(ids), -1)


@GROUPS
def test_ragged_batches_one_base_per_lane(eng, oracle, tables, g2):
    counts = [16, 16, 1, 5, 0, 16]
    ids = [oc.o.bench_scalar("openings_gpu17", i) for i in range(sum(counts))]
    B = powers(eng, g2, 17)
    assert B.tobytes() == oc.bases(g2, 17).tobytes()
    want, want_ok, _ = oc.expected(oracle, g2, ids, counts, 17)
    assert want_ok.all() and want.any(1).all()
    for form, coeffs, pts, ok in both_forms(eng, tables[g2, 17], ids, counts):
        assert coeffs.tobytes() == oc.coeff_rows([v % R for v in ids], counts, 17).tobytes(), form
        assert ok.tolist() == want_ok.tolist() and pts.tobytes() == want.tobytes(), form
        assert pts[32].tobytes() == B[0].tobytes(), form                                  # the batch of one: q = 1


@GROUPS
def test_the_corpus_on_the_device(eng, oracle, tables, g2):
    """every segment length from 0 to nbase - 1, the residues, the repeated identity and tau among the identities"""
    ids, counts, names, want, want_ok, _ = oc.expected_corpus(oracle, g2)
    for form, coeffs, pts, ok in both_forms(eng, tables[g2, oc.NBASE[g2]], ids, counts):
        assert coeffs.tobytes() == oc.coeff_rows([v % R for v in ids], counts, oc.NBASE[g2]).tobytes(), form
        assert ok.tolist() == want_ok.tolist() and pts.tobytes() == want.tobytes(), form
        rep, tau = oc.rows_of(counts, names, "repeated"), oc.rows_of(counts, names, "tau")
        assert ok[rep].tolist() == [0, 1, 0] and not pts[rep[0]].any() and not pts[rep[2]].any() and pts[rep[1]].any(), form
        assert ok[tau].tolist() == [1, 1, 1] and not pts[tau[0]].any() and not pts[tau[2]].any() and pts[tau[1]].any(), form
    K = oc.scalar_rows(ids)
    pts, ok = tables[g2, oc.NBASE[g2]].openings(to_dev(K), counts, out=to_dev(np.full_like(want, 0xA5)), ok_out=to_dev(np.full(len(ids), 0xA5, np.uint8)))
    assert pts.cpu().numpy().tobytes() == want.tobytes() and ok.cpu().numpy().tolist() == want_ok.tolist()


def existing_route(eng, table, K, B):
    """fr_poly_from_roots + fr_poly_quotients + FixedBase.msm on whole batches of B: (coeffs, points, ok)"""
    coeffs = eng.fr_poly_from_roots(K, B)
    q, ok = eng.fr_poly_quotients(coeffs.reshape(-1), K, B, table.nbase)
    return coeffs, table.msm(q.reshape(-1)), ok


@GROUPS
def test_full_batches_equal_the_existing_route(eng, tables, g2):
    """8 batches of 256 under 257 bases: four bases per lane, 65 chunks, two levels; one identity repeated in the last batch, which the
    existing route accepts (the quotient is exact) and the fused entry refuses on both copies"""
    B, k = 256, 8
    ids = [oc.o.bench_scalar("openings_gpu257", i) for i in range(B * k)]
    ids[7 * B + 200] = ids[7 * B + 3]
    K, table = oc.scalar_rows(ids), tables[g2, 257]
    for put, back in ((lambda a: a, np.asarray), (to_dev, lambda a: a.cpu().numpy())):
        old_coeffs, old_pts, old_ok = (back(x) for x in existing_route(eng, table, put(K), B))
        coeffs = back(eng.fr_poly_from_roots_segments(put(K), B, B + 1))
        assert coeffs.tobytes() == old_coeffs.tobytes()
        pts, ok = (back(x) for x in table.openings(put(K), [B] * k))
        assert old_ok.all()
        dup = [7 * B + 3, 7 * B + 200]
        assert ok[dup].tolist() == [0, 0] and not pts[dup].any() and ok.sum() == B * k - 2
        keep = np.ones(B * k, dtype=bool)
        keep[dup] = False
        assert pts[keep].tobytes() == old_pts.reshape(B * k, -1)[keep].tobytes()
    assert pts[:B].tobytes() == at_tau(eng, g2, ids[:B]).tobytes()


def test_a_long_batch_takes_the_large_staging(eng, tables):
    """G1, 300 bases, batches of 299 and 3: segments above 256 run the instance with 1025 coefficients in LDS"""
    ids = [oc.o.bench_scalar("openings_gpu300", i) for i in range(302)]
    K, table = oc.scalar_rows(ids), tables[False, 300]
    _, old_pts, old_ok = existing_route(eng, table, K[:299 * 32], 299)
    assert old_ok.all()
    short = at_tau(eng, False, ids[299:])
    for form, coeffs, pts, ok in both_forms(eng, table, ids, [299, 3]):
        assert ok.all(), form
        assert pts[:299].tobytes() == np.asarray(old_pts).tobytes() and pts[299:].tobytes() == short.tobytes(), form
        assert not coeffs[1, 4:].any() and coeffs[0, 299].tobytes() == (1).to_bytes(32, "little"), form


def test_calls_in_flight_keep_their_own_segment_tables(eng, tables):
    """24 calls with 24 different segment tables enqueued back to back on a side stream, nothing waited for in between: every call works
    on the table it was given (the library copies it before it returns, through a ring of eight pinned buffers that is gone round three
    times here), and the results are those of the host form"""
    import torch
    ids = [oc.o.bench_scalar("openings_gpu17", i) for i in range(54)]
    K, table = oc.scalar_rows(ids), tables[False, 17]
    variants = []
    for t in range(24):
        cuts = sorted({(7 * t + 5 * j) % 54 for j in range(1 + t % 6)} | {0, 54})
        counts = [b - a for a, b in zip(cuts, cuts[1:])]
        counts = [c for m in counts for c in ([16] * (m // 16) + [m % 16])]                # no batch above nbase - 1 = 16; zeros stay in
        variants.append(counts)
        assert sum(counts) == 54 and max(counts) <= 16
    assert len({tuple(v) for v in variants}) >= 12
    want = [table.openings(K, counts) for counts in variants]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dK = to_dev(K)
        got = [table.openings(dK, counts) + (eng.fr_poly_from_roots_segments(dK, counts, 17),) for counts in variants]
    side.synchronize()
    for counts, (pts, ok), (dpts, dok, dco) in zip(variants, want, got):
        assert dpts.cpu().numpy().tobytes() == pts.tobytes() and dok.cpu().numpy().tolist() == ok.tolist(), counts
        assert dco.cpu().numpy().tobytes() == oc.coeff_rows([v % R for v in ids], counts, 17).tobytes(), counts
