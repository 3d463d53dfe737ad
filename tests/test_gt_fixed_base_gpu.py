"""Fixed-base exponentiation in GT on the MI355X (run with -m gpu): k_gt_fb_build and k_gt_fb_indexed through bn254.GTFixedBase, that is
through the C entries of include/gpbc_bn254_gtfixed.h in the host form and the _dev form.  Everything is bit-exact.  Every output is held

  * against the C oracle (gt_exp per term, gt_mul in term order) — never against the code under test — and, for the exponent corpus,
    against the Python integers of tests/gt_fixed_cases.py as well;
  * against gpbc_gt_exp_batch (+ gt_mul) on the same inputs: the route the table replaces, an independent device path.

Bases: one, e(g1, g2), a Miller-loop value (not cyclotomic), zero; nbase = 1 and 4.  Shapes: n in {1, 31, 32, 33, 65} (a wavefront holds 32
lane pairs), terms in {1, 2, 16}, n_index_rows = n, 1, and 3 with n = 65.  Rows: a base under k and r - k, a row of only INDEX_NONE, an
index equal to nbase between untouched neighbours.  Two handles alive at once."""
import numpy as np
import pytest

import gt_fixed_cases as gc

pytestmark = pytest.mark.gpu
GUARD = 0xA5


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


@pytest.fixture(scope="module")
def tables(eng):
    """{nbase: GTFixedBase}: the one-base table from host bases, the four-base table from a CUDA tensor — both alive for the whole module"""
    t = {1: eng.GTFixedBase(gc.bases()[gc.PAIRING]), 4: eng.GTFixedBase(to_dev(gc.bases()))}
    yield t
    for table in t.values():
        table.close()


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def base_rows(nbase):
    return gc.bases()[gc.PAIRING:gc.PAIRING + 1] if nbase == 1 else gc.bases()


def by_terms(oracle_or_eng, nbase, index, scalars, n):
    """(out, ok) from gt_exp per term and gt_mul in term order, on `oracle_or_eng` (the C oracle, or the engine's own gt_exp / gt_mul):
    a term that is NONE contributes one, a row with an index >= nbase is all zero with ok = 0"""
    from gopairingbasedcryptography_amd._plan import GT_ONE
    B, terms = base_rows(nbase), len(index[0])
    rows = [index[i % len(index)] for i in range(n)]
    ok = np.array([all(j == gc.NONE or j < nbase for j in row) for row in rows], dtype=np.uint8)
    acc = np.tile(GT_ONE, (n, 1))
    for t in range(terms):
        live = [i for i in range(n) if ok[i] and rows[i][t] != gc.NONE]
        if not live:
            continue
        x = np.stack([B[rows[i][t]] for i in live])
        k = gc.scalar_rows([scalars[i][t] for i in live])
        power = np.tile(GT_ONE, (n, 1))
        power[live] = np.asarray(oracle_or_eng.gt_exp(x.reshape(-1), k.reshape(-1))).reshape(-1, 384)
        acc = np.asarray(oracle_or_eng.gt_mul(acc.reshape(-1), power.reshape(-1))).reshape(n, 384)
    acc[ok == 0] = 0
    return acc, ok


def run_both_forms(table, index, scalars, terms):
    """the host form and the _dev form of one call: [(form, out, ok)] as host arrays"""
    import torch
    idx, K = gc.index_array(index), gc.scalar_rows([k for row in scalars for k in row])
    out, ok = table.indexed(idx, K, terms=terms)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and isinstance(ok, np.ndarray)
    dout, dok = table.indexed(to_dev(idx.view(np.int32)), to_dev(K), terms=terms)
    assert dout.is_cuda and dout.dtype == torch.uint8 and dok.is_cuda
    return [("host", out, ok), ("device", dout.cpu().numpy(), dok.cpu().numpy())]


def check(eng, oracle, table, nbase, index, scalars, n, what):
    terms = len(index[0])
    want, want_ok = by_terms(oracle, nbase, index, scalars, n)
    other, other_ok = by_terms(eng, nbase, index, scalars, n)
    assert other.tobytes() == want.tobytes() and other_ok.tolist() == want_ok.tolist(), (what, "gt_exp_batch route against the oracle")
    for form, out, ok in run_both_forms(table, index, scalars, terms):
        assert out.shape == (n, 384) and ok.shape == (n,)
        assert ok.tolist() == want_ok.tolist(), (what, form)
        bad = np.nonzero((out != want).any(1))[0]
        assert not bad.size, (what, form, bad.tolist(), [index[i % len(index)] for i in bad[:4]], [[hex(k) for k in scalars[i]] for i in bad[:4]])
    return want, want_ok


@pytest.mark.parametrize("nbase", [1, 4])
def test_every_exponent_on_every_base(eng, oracle, tables, nbase):
    """0, 1, 255, 256, 2^(8w), 2^256 - 1, a lone top digit, r - 1, r, r + 1 and stream scalars on one, e(g1, g2), a Miller value and zero:
    the scalar is used as the integer it is, whatever the order of the base; zero^0 = one, zero^k = zero"""
    index, scalars, n = gc.every_base_every_exponent(nbase)
    if nbase == 1:
        values = gc.base_values()[gc.PAIRING:gc.PAIRING + 1]
        ints = gc.gt_rows([gc.o.f12_pow(values[0], k[0]) for k in scalars])
    else:
        ints = gc.expected(index, scalars, n, nbase)[0]
    want, _ = check(eng, oracle, tables[nbase], nbase, index, scalars, n, "nbase = %d" % nbase)
    assert want.tobytes() == ints.tobytes()                                                 # the C oracle and the Python integers agree
    if nbase == 4:
        E = len(gc.EXPONENTS)
        from gopairingbasedcryptography_amd._plan import GT_ONE
        assert want[gc.ZERO * E].tobytes() == GT_ONE.tobytes() and not want[gc.ZERO * E + 1:].any()      # zero^0, then zero^k
        assert want[gc.PAIRING * E + gc.EXPONENTS.index(gc.o.R)].tobytes() == GT_ONE.tobytes()             # e(g1, g2)^r
        assert want[gc.MILLER * E + gc.EXPONENTS.index(gc.o.R)].tobytes() != GT_ONE.tobytes()              # ... but not a Miller value's


@pytest.mark.parametrize("n,terms,rows", [(n, terms, n) for n in (1, 31, 32, 33, 65) for terms in (1, 2, 16)]
                         + [(33, 1, 1), (65, 2, 1), (65, 1, 3), (65, 16, 3)])
def test_shapes_terms_and_periodic_rows(eng, oracle, tables, n, terms, rows):
    """sizes at the wavefront edge, 1 / 2 / 16 terms, every output its own index row, one row for all, and three rows with n = 65 (no
    multiple); with own rows the call holds the row of only INDEX_NONE, the row with an index equal to nbase (zero, ok = 0, its neighbours
    as the oracle has them) and, from two terms on, the row of one base under k and r - k"""
    from gopairingbasedcryptography_amd._plan import GT_ONE
    index, scalars = gc.shaped(n, terms, rows, 4)
    want, ok = check(eng, oracle, tables[4], 4, index, scalars, n, (n, terms, rows))
    if rows == n and n >= 2:
        assert want[1].tobytes() == GT_ONE.tobytes()
    if rows == n and n >= 5:
        assert ok.tolist() == [1, 1, 1, 0] + [1] * (n - 4) and not want[3].any() and want[2].any() and want[4].any()
    if rows == n and n >= 7 and terms >= 2:
        assert want[5].tobytes() == GT_ONE.tobytes() and index[5][:2] == [gc.PAIRING, gc.PAIRING]


@pytest.mark.parametrize("n", [1, 33])
def test_one_base_table_and_pow(eng, oracle, tables, n):
    """nbase = 1: pow() against gt_exp of the oracle and of the device on the replicated base, host and device scalars, a caller's out
    with guards round it"""
    import torch
    E = gc.EXPONENTS
    ks = [E[(7 * i + 2) % len(E)] for i in range(n)]
    K = gc.scalar_rows(ks)
    x = np.tile(gc.bases()[gc.PAIRING], (n, 1))
    want = np.asarray(oracle.gt_exp(x.reshape(-1), K.reshape(-1))).reshape(n, 384)
    assert np.asarray(eng.gt_exp(x.reshape(-1), K.reshape(-1))).reshape(n, 384).tobytes() == want.tobytes()
    assert tables[1].pow(ks).tobytes() == want.tobytes() and tables[1].pow(K).tobytes() == want.tobytes()
    assert tables[4].pow(K, base=gc.PAIRING).tobytes() == want.tobytes()
    buf = torch.full((n * 384 + 64,), GUARD, dtype=torch.uint8, device="cuda")
    out = tables[1].pow(to_dev(K), out=buf[32:32 + n * 384])
    assert out.data_ptr() == buf.data_ptr() + 32 and out.cpu().numpy().tobytes() == want.tobytes()
    assert bool((buf[:32] == GUARD).all()) and bool((buf[32 + n * 384:] == GUARD).all())
    hout, hok = np.full(n * 384 + 8, GUARD, np.uint8), np.full(n + 8, GUARD, np.uint8)
    tables[1].indexed(np.zeros(1, np.uint32), K, terms=1, out=hout[:n * 384], ok_out=hok[:n])
    assert hout[:n * 384].tobytes() == want.tobytes() and (hok[:n] == 1).all() and (hout[n * 384:] == GUARD).all() and (hok[n:] == GUARD).all()


def test_two_handles_destroy_one_reuse_the_other(eng, oracle):
    """two tables built one after the other hold different bases; closing the first leaves the second as it was, and a closed table is
    refused before any C call"""
    B = gc.bases()
    a, b = eng.GTFixedBase(B[gc.MILLER]), eng.GTFixedBase(to_dev(B[[gc.PAIRING, gc.MILLER]]))
    assert a.table_bytes() == 4 << 20 and b.table_bytes() == 8 << 20
    ks = gc.EXPONENTS[7:12]
    K = gc.scalar_rows(ks)
    want = np.asarray(oracle.gt_exp(np.tile(B[gc.MILLER], (len(ks), 1)).reshape(-1), K.reshape(-1))).reshape(-1, 384)
    assert a.pow(ks).tobytes() == want.tobytes() and b.pow(ks, base=1).tobytes() == want.tobytes()
    a.close()
    a.close()                                                                               # twice is harmless
    assert b.pow(to_dev(K), base=1).cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="closed"):
        a.pow(ks)
    c = eng.GTFixedBase(B[gc.PAIRING])                                                      # a new table where the old one was freed
    assert b.pow(ks, base=1).tobytes() == want.tobytes()
    assert c.pow([1]).tobytes() == B[gc.PAIRING].tobytes()
    b.close()
    c.close()


def test_empty_calls_and_argument_errors_on_the_device(eng, tables):
    import torch
    out, ok = tables[4].indexed(np.zeros(2, np.uint32), np.zeros(0, np.uint8), terms=2)
    assert out.shape == (0, 384) and ok.shape == (0,)
    out, ok = tables[4].indexed(torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.uint8, device="cuda"), terms=2)
    assert out.is_cuda and tuple(out.shape) == (0, 384)
    lib = tables[4]._lib
    buf = torch.zeros(4 * 384 + 4 * 32, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    # out begins inside the scalars: refused with nothing launched
    assert lib.gpbc_gt_fixed_base_indexed_dev(tables[4]._h, idx.data_ptr(), 4, 1, buf.data_ptr(), 4, buf.data_ptr() + 4 * 32 - 1, None, None) == -1
    assert b"overlaps" in lib.gpbc_last_error()
    assert lib.gpbc_gt_fixed_base_indexed_dev(tables[4]._h, idx.data_ptr(), 5, 1, buf.data_ptr(), 4, buf.data_ptr() + 4 * 32, None, None) == -1
    torch.cuda.synchronize()
    assert not bool(buf.any())
    with pytest.raises(ValueError):
        eng.GTFixedBase(np.zeros(383, np.uint8))
    with pytest.raises(ValueError):
        eng.GTFixedBase(np.zeros(0, np.uint8))
    with pytest.raises(ValueError, match="base must be"):
        tables[4].pow([1], base=4)
