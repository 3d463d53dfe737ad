"""The corpus of the opening-proof tests (tests/test_openings.py on the host interval build, tests/test_openings_gpu.py on the device):
identities in ragged batches, their batch polynomials and quotients in Python integers, and the expected points from the C oracle's scalar
multiplications and sums — one multiplication per (coefficient, base [tau^c]) and one sum per identity, as the reference's
computeG1/G2PolynomialTau does it.  Computed once per process and shared.

  segments   lengths 0, 1, 2, 3 and nbase - 1 mixed in one call; the length-1 segment has q = 1, so its opening is base 0
  residues   0, r - 1, and a value >= r equal to another identity of its batch modulo r: those two rows get ok = 0, the others ok = 1
  repeated   a batch with one identity twice: both copies ok = 0 and zero rows, the third identity untouched
  tau        tau itself among the identities: the digest is infinity, every other opening of the batch is the all-zero point with ok = 1,
             and the opening of tau is not zero — the sum of the chain passes through infinity"""
import functools

import numpy as np

import bn254_py as o

R = o.R
TAU = o.bench_scalar("openings_tau", 0) % R
NBASE = {False: 9, True: 5}                                          # G1 table of 9 bases, G2 table of 5


def scalar_rows(values):
    """Python integers below 2^256 as they are: flat uint8, 32 bytes each, little-endian"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).copy()


@functools.lru_cache(maxsize=None)
def bases(g2, nbase=None):
    """[nbase, 64|128] uint8: [tau^c] of the group's generator, c = 0 .. nbase - 1, in Python integers"""
    nbase = NBASE[g2] if nbase is None else nbase
    if g2:
        return np.stack([np.frombuffer(o.g2_to_bytes(o.g2_mul(o.G2_GEN, pow(TAU, c, R))), dtype=np.uint8) for c in range(nbase)])
    return np.stack([np.frombuffer(o.g1_to_bytes(o.g1_mul(o.G1_GEN, pow(TAU, c, R))), dtype=np.uint8) for c in range(nbase)])


def _fresh(tag, count):
    return [o.bench_scalar(tag, i) % R for i in range(count)]


@functools.lru_cache(maxsize=None)
def corpus(nbase):
    """(ids, counts, names): the identities of one call as Python integers below 2^256, the batch sizes, and what each batch is for"""
    full = nbase - 1
    x = _fresh("openings_x", 2)
    rep = _fresh("openings_rep", 2)
    other = _fresh("openings_tau_batch", 2)
    batches = [
        ("empty", []),
        ("one", _fresh("openings_one", 1)),
        ("two", _fresh("openings_two", 2)),
        ("three", _fresh("openings_three", 3)),
        ("full", _fresh("openings_full", full)),
        ("residues", [0, R - 1, x[0], x[0] + R]),
        ("repeated", [rep[0], rep[1], rep[0]]),
        ("tau", [other[0], TAU, other[1]]),
        ("empty again", []),
    ]
    assert all(len(b) <= full for _, b in batches)
    return [v for _, b in batches for v in b], [len(b) for _, b in batches], [name for name, _ in batches]


def poly_from_roots(roots):
    """coefficients of prod (X - root) modulo r, constant term first"""
    c = [1]
    for root in roots:
        c = [((c[i - 1] if i else 0) - root * (c[i] if i < len(c) else 0)) % R for i in range(len(c) + 1)]
    return c


def quotient(f, root):
    """(q, remainder) of f / (X - root) modulo r"""
    q, carry = [0] * (len(f) - 1), 0
    for i in range(len(f) - 1, 0, -1):
        carry = (f[i] + carry * root) % R
        q[i - 1] = carry
    return q, (f[0] + carry * root) % R


def segments(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def coeff_rows(ids, counts, stride):
    """[k * stride * 32] uint8: the rows gpbc_fr_poly_from_roots_segments writes"""
    seg = [int(v) for v in segments(counts)]
    rows = []
    for a, b in zip(seg, seg[1:]):
        f = poly_from_roots(ids[a:b])
        rows += f + [0] * (stride - len(f))
    return scalar_rows(rows)


def expected(oracle, g2, ids, counts, nbase=None):
    """(points [n, 64|128], ok [n], q) in Python integers and oracle group operations; q[i] = the quotient's coefficients of identity i
    (None where ok = 0).  An identity is ok iff exactly one identity of its batch equals it modulo r (the reference's rule)."""
    B = bases(g2, nbase)
    width = B.shape[1]
    mul, add = (oracle.g2_scalar_mul, oracle.g2_sum) if g2 else (oracle.g1_scalar_mul, oracle.g1_sum)
    seg = [int(v) for v in segments(counts)]
    pts, ok, qs = np.zeros((len(ids), width), dtype=np.uint8), np.zeros(len(ids), dtype=np.uint8), [None] * len(ids)
    for a, b in zip(seg, seg[1:]):
        batch = [v % R for v in ids[a:b]]
        f = poly_from_roots(batch)
        for i in range(a, b):
            if batch.count(ids[i] % R) != 1:
                continue
            q, rem = quotient(f, ids[i] % R)
            assert rem == 0
            ok[i], qs[i] = 1, q
            live = [c for c, v in enumerate(q) if v]
            if live:
                terms = np.asarray(mul(B[live].reshape(-1), scalar_rows([q[c] for c in live]))).reshape(-1, width)
                terms = terms[terms.any(1)]
                if len(terms):
                    pts[i] = np.asarray(add(terms.reshape(-1))).reshape(width)
    return pts, ok, qs


_CACHE = {}


def expected_corpus(oracle, g2, nbase=None):
    """expected() on corpus(nbase), once per process: (ids, counts, names, points, ok, q)"""
    nbase = NBASE[g2] if nbase is None else nbase
    key = (g2, nbase)
    if key not in _CACHE:
        ids, counts, names = corpus(nbase)
        _CACHE[key] = (ids, counts, names) + expected(oracle, g2, ids, counts, nbase)
    return _CACHE[key]


def rows_of(counts, names, name):
    """the identity positions of the batch called `name`"""
    j = names.index(name)
    a = sum(counts[:j])
    return list(range(a, a + counts[j]))
