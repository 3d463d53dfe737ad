"""Test helper: what the G2 row tables (csrc/rows29_g2.hip.hpp) are run on beyond the case table of tests/rows_cases.py, whose bases,
planted scalars and expectations (the oracle's scalar multiplication on the bases expanded per scalar) the G2 tests share.

A split is (k0, k1, k2, k3, n0, n1, n2, n3): four magnitudes and four signs, standing for the scalar sum +-k_i mu^i, mu = 6 u^2 the
eigenvalue of psi on the order-r subgroup of the twist (= p modulo r).  gls_split reaches few sign patterns and no chosen digits, so the
walk is given its splits directly:
  SINGLES        one nibble per (quarter, window), all 68, each under both signs; window 16 holds two bits, its digit is at most 3
  FULL           every quarter 2^66 - 1 under all 16 sign patterns
  ZERO           nothing to add
  CANCEL         (u + 1) + u mu + u mu^2 - 2 u mu^3 = 0 modulo r (the relation behind the subgroup test of csrc/wire29.hip.hpp): the walk
                 reaches the point at infinity at its LAST addition, an exceptional branch of jac_add_mixed; with 16^16 added to quarter 0
                 — its window 16 comes after the others — the walk reaches infinity and starts again: [2^64] P
and SCALARS_MU are d 16^w mu^i for every (i, w), which go through gls_split."""
import random

import numpy as np

import bn254_py as o

R = o.R
MU = 6 * o.U * o.U % R
assert MU == o.P % R and (pow(MU, 4, R) - pow(MU, 2, R) + 1) % R == 0
WINDOWS, QUARTER_MAX = 17, (1 << 66) - 1


def _digit(i, w):
    return min(1 + (7 * w + 3 * i) % 15, 3 if w == 16 else 15)


def _one(i, v, neg):
    k, n = [0, 0, 0, 0], [0, 0, 0, 0]
    k[i], n[i] = v, neg
    return tuple(k + n)


SINGLES = [_one(i, _digit(i, w) << (4 * w), neg) for i in range(4) for w in range(WINDOWS) for neg in (0, 1)]
FULL = [(QUARTER_MAX,) * 4 + tuple((s >> i) & 1 for i in range(4)) for s in range(16)]
ZERO = [(0,) * 8]
CANCEL = [(o.U + 1, o.U, o.U, 2 * o.U, 0, 0, 0, 1), (o.U + 1, o.U, o.U, 2 * o.U, 1, 1, 1, 0),
          (o.U + 1 + (1 << 64), o.U, o.U, 2 * o.U, 0, 0, 0, 1), (o.U + 1 + (3 << 64), o.U, o.U, 2 * o.U, 1, 1, 1, 0)]
SPLITS = SINGLES + FULL + ZERO + CANCEL
SCALARS_MU = [(_digit(i, w) << (4 * w)) * pow(MU, i, R) % R for i in range(4) for w in range(WINDOWS)]


def split_scalar(s):
    return sum((-k if n else k) * pow(MU, i, R) for i, (k, n) in enumerate(zip(s[:4], s[4:]))) % R


def split_rows(splits):
    """splits -> the 16 uint32 per split of rg_eval_split / rg_gls_split: 3 words per quarter, then the four signs"""
    return np.array([[(k >> (32 * t)) & 0xFFFFFFFF for k in s[:4] for t in range(3)] + list(s[4:]) for s in splits], dtype=np.uint32)


def rows_split(row):
    """one row of rg_gls_split -> a split"""
    r = [int(v) for v in row]
    return tuple(r[3 * i] | r[3 * i + 1] << 32 | r[3 * i + 2] << 64 for i in range(4)) + tuple(r[12:16])


assert [split_scalar(s) for s in CANCEL] == [0, 0, (1 << 64) % R, -(3 << 64) % R]


def random_scalars(n, seed=0):
    rnd = random.Random(31337 + seed)
    return [rnd.randrange(1 << 256) for _ in range(n)]
