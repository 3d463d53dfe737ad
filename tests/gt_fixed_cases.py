"""The corpus of the fixed-base GT tests (tests/test_gt_fixed_base.py on the host interval build, tests/test_gt_fixed_base_gpu.py on the
device): bases, exponents, index rows and their expected outputs, all in Python integers (oracle/bn254_py.py).  Computed once per process.

  bases      one; e(g1, g2), cyclotomic and of order r; a Miller-loop value, a unit outside the cyclotomic subgroup; zero
  exponents  0, 1, 255, 256; 2^(8w) for w = 1, 15, 31; every digit 255 (2^256 - 1); a single non-zero top digit; r - 1, r, r + 1;
             scalars of the SURVEY section 8d stream
  rows       the same order-r base twice under k and r - k (one); only INDEX_NONE (one); an index equal to nbase (zero row, ok = 0)"""
import functools

import numpy as np

import bn254_py as o

NONE = 0xFFFFFFFF
ONE, PAIRING, MILLER, ZERO = 0, 1, 2, 3                               # positions in bases()
F12_ZERO = (o.F6_ZERO, o.F6_ZERO)


@functools.lru_cache(maxsize=None)
def base_values():
    return [o.F12_ONE, o.pair([o.G1_GEN], [o.G2_GEN]), o.miller_loop(o.g1_mul(o.G1_GEN, 5), o.g2_mul(o.G2_GEN, 7)), F12_ZERO]


def gt_rows(values):
    return np.stack([np.frombuffer(o.gt_to_bytes(v), dtype=np.uint8) for v in values])


def bases():
    """[4, 384] uint8: one, e(g1, g2), a Miller value, zero"""
    return gt_rows(base_values())


EXPONENTS = ([0, 1, 255, 256] + [1 << (8 * w) for w in (1, 15, 31)] + [(1 << 256) - 1, 0xC3 << 248, o.R - 1, o.R, o.R + 1]
             + [o.bench_scalar("gt_fixed", i) for i in range(3)])


def scalar_rows(values):
    """Python integers below 2^256 as they are: [len, 32] uint8, little-endian"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32).copy()


@functools.lru_cache(maxsize=None)
def _power(j, k):
    return o.f12_pow(base_values()[j], k)


def expected(index, scalars, n, nbase):
    """(out [n, 384], ok [n]) of an indexed product in Python integers: index a list of rows (NONE for no term), periodic when shorter than
    n; scalars a list of n rows of integers; an index >= nbase other than NONE gives a zero row and ok = 0"""
    out, ok = np.zeros((n, 384), dtype=np.uint8), np.ones(n, dtype=np.uint8)
    for i in range(n):
        row = index[i % len(index)]
        if any(j != NONE and j >= nbase for j in row):
            ok[i] = 0
            continue
        acc = o.F12_ONE
        for j, k in zip(row, scalars[i]):
            if j != NONE:
                acc = o.f12_mul(acc, _power(j, k))
        out[i] = np.frombuffer(o.gt_to_bytes(acc), dtype=np.uint8)
    return out, ok


def index_array(index):
    return np.array([j for row in index for j in row], dtype=np.uint32)


def every_base_every_exponent(nbase):
    """terms = 1, n_index_rows = n: every exponent of EXPONENTS on every one of the first nbase bases -> (index, scalars, n)"""
    index = [[j] for j in range(nbase) for _ in EXPONENTS]
    scalars = [[k] for _ in range(nbase) for k in EXPONENTS]
    return index, scalars, len(index)


def shaped(n, terms, n_index_rows, nbase, special=True):
    """A call of n outputs with `terms` terms and n_index_rows index rows over the first nbase bases, every output with exponents of its
    own drawn from EXPONENTS in turn.  With own rows (n_index_rows == n) and special, the last three rows that fit are the cancelling row
    (base PAIRING under k and r - k; needs terms >= 2 and nbase > PAIRING), the row of only NONE, and the row with an index equal to
    nbase between two ordinary neighbours."""
    E = EXPONENTS
    index = [[(i + 2 * t) % min(nbase, ZERO) for t in range(terms)] for i in range(n_index_rows)]       # one, e(g1, g2) and the Miller value mixed ...
    for i in range(6, n_index_rows, 8):
        index[i][0] = nbase - 1                                                                          # ... and now and then the zero base
    scalars = [[E[(5 * i + 3 * t) % len(E)] for t in range(terms)] for i in range(n)]
    if special and n_index_rows == n:
        if n >= 2:
            index[1] = [NONE] * terms
        if n >= 5:
            index[3] = [nbase] + index[3][1:]
        if n >= 7 and terms >= 2 and nbase > PAIRING:
            k = o.bench_scalar("gt_fixed_cancel", 0)
            index[5] = [PAIRING, PAIRING] + [NONE] * (terms - 2)
            scalars[5] = [k, o.R - k] + scalars[5][2:]
    elif special and n_index_rows >= 2:
        index[1] = [NONE] + index[1][1:]
    return index, scalars
