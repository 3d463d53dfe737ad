"""Test helper: the case table of the row form of g1 / g2_scalar_mul (out[j m + i] = [k_(j m + i)] base_j, csrc/rows29.hip.hpp) with what
it must give — the oracle's scalar multiplication on the bases expanded per scalar.  Shared by the host-harness test
(test_scalar_mul_rows.py) and the GPU tests; an expectation is computed once per (group, shape) and kept.

What is planted, and where.  Bases: the generator first, the point at infinity second (between two ordinary ones wherever there are
three bases), random multiples of the generator after it.  Scalars, on the rows of ordinary bases in this order, as many as fit:
0, 1, 2, r - 1, r, r + 1, 2^128 - 1, 2^128, 2^256 - 1; the GLV eigenvalue lambda and lambda +- 1; 2^124 - 1 (half one all nibbles 15
up to where glv_split reaches) and (2^128 - 1)(1 + lambda); then per window w the scalar d 16^w — its split IS the single nibble (w, d) of
half one while it stays below 2^256 / g2, which caps d at 6 in window 31 — and the scalar d 16^w lambda, which a single nibble of half two
stands for.  The rest is random below 2^256.

glv_split itself never returns k1 < 0, and k2 > 0 only with k1 (split() below restates it; its comment has the reason), so the splits
whose signs, windows and digits the evaluation has to get right are given to it directly: SPLITS is the list (k1, k2, neg1, neg2) with
the 64 single nibbles, one per window of each half, every nibble 15 in both halves, and all four sign combinations of each; the
scalar such a split stands for is split_scalar()."""
import os
import random
import re

import numpy as np

import bn254_py as o
from conftest import ROOT

R = o.R
TOP = (1 << 256) - 1
G1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
G2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
SHAPES = [(3, 65), (65, 3), (2, 16)]                      # (nbase, m) of the host-harness test; the GPU tests add theirs


def rows(vals):
    """ints below 2^256, NOT reduced -> [n, 32] scalar rows"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


# ---- glv_split of csrc/curve29.hip.hpp in Python integers, from the constants the kernels use
def _constant(name):
    with open(os.path.join(ROOT, "gopairingbasedcryptography_amd", "csrc", "bn254_constants29.hip.hpp")) as f:
        words = re.search(r"#define %s \{([^}]*)\}" % name, f.read()).group(1)
    return sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(words.split(",")))


_G1C, _G2C, _A1, _A2, _B1, _B2 = (_constant("GLV_" + n) for n in ("G1", "G2", "A1", "A2", "B1ABS", "B2"))
assert _constant("GLV_R32") == R


def split(k):
    """(k1, k2, neg1, neg2), magnitudes and signs.  c_i = floor(k g_i / 2^256) with both g_i BELOW 2^256 b / r, so c_i never exceeds the
    exact quotient: k1 = e1 a1 + e2 a2 with e >= 0 is never negative, and k2 = e2 b2 - e1 |b1| is positive only while e1 |b1| < e2 b2,
    which is k below about 2^127."""
    k %= R
    c1, c2, M = (k * _G1C) >> 256, (k * _G2C) >> 256, 1 << 160
    r1, r2 = (k - c1 * _A1 - c2 * _A2) % M, (c1 * _B1 - c2 * _B2) % M
    n1, n2 = r1 >> 159, r2 >> 159
    return (M - r1) % M if n1 else r1, (M - r2) % M if n2 else r2, n1, n2


def _eigenvalue():
    """the cube root of unity modulo r that glv_split splits along: k = +-k1 +- k2 lambda"""
    root = next(pow(g, (R - 1) // 3, R) for g in (2, 3, 5, 7, 11) if pow(g, (R - 1) // 3, R) != 1)
    k = 0x1234567890ABCDEF << 180
    k1, k2, n1, n2 = split(k)
    return next(c for c in (root, root * root % R) if ((-k1 if n1 else k1) + (-k2 if n2 else k2) * c - k) % R == 0)


LAMBDA = _eigenvalue()
HALF_ONE_MAX = (1 << 256) // _G2C                         # below this c2 = 0 (and c1 = 0): split(k) = (k, 0)


def split_scalar(s):
    k1, k2, n1, n2 = s
    return ((-k1 if n1 else k1) + (-k2 if n2 else k2) * LAMBDA) % R


def _digit(w, h):
    d = 1 + (7 * w + 3 * h) % 15
    return min(d, 6) if w == 31 and not h else d


def _splits():
    out = []
    for h in (0, 1):
        for w in range(32):
            v = _digit(w, h) << (4 * w)
            out.append((0, v, (w >> 1) & 1, w & 1) if h else (v, 0, w & 1, (w >> 1) & 1))
    full = (1 << 128) - 1
    out += [(full, full, a, b) for a in (0, 1) for b in (0, 1)]
    out += [(15 << 124 | 1, 1 << 124 | 15, a, b) for a in (0, 1) for b in (0, 1)]
    out += [(0, 0, 0, 0), (1, 1, 0, 1), (1, 1, 1, 0)]                    # nothing to add; P + phi(P) + ... cancellations: P - phi(P), -P + phi(P)
    return out


SPLITS = _splits()
SPECIAL = [0, 1, 2, R - 1, R, R + 1, (1 << 128) - 1, 1 << 128, TOP, LAMBDA, LAMBDA + 1, LAMBDA - 1, (1 << 124) - 1, ((1 << 128) - 1) * (1 + LAMBDA) % R]
SINGLES = [v for w in range(32) for v in ((_digit(w, 0) << (4 * w)), (_digit(w, 1) << (4 * w)) * LAMBDA % R)]
PLANTED = SPECIAL + SINGLES
INF_BASE = 1


def scalars(nbase, m, seed=0):
    """the n = nbase m scalars of a shape: PLANTED along the rows of the ordinary bases, random below 2^256 elsewhere"""
    rnd = random.Random(977 * nbase + m + seed)
    ks = [rnd.randrange(1 << 256) for _ in range(nbase * m)]
    slots = [j * m + i for j in range(nbase) if not (nbase >= 3 and j == INF_BASE) for i in range(m)]
    for at, v in zip(slots, PLANTED):
        ks[at] = v
    return ks


_bases, _expected = {}, {}


def bases(oracle, g2, nbase):
    """[nbase, 64 | 128]: the generator, the point at infinity (from three bases on), random multiples of the generator"""
    if (g2, nbase) not in _bases:
        ks = [1] + [o.bench_scalar("rows-base", i) for i in range(1, nbase)]
        b = np.asarray((oracle.g2_scalar_mul if g2 else oracle.g1_scalar_mul)(G2 if g2 else G1, rows(ks), threads=8)).reshape(nbase, -1).copy()
        if nbase >= 3:
            b[INF_BASE] = 0
        _bases[(g2, nbase)] = b
    return _bases[(g2, nbase)]


def expand(b, m):
    """the bases repeated m times each: what the nbase == n call takes"""
    return np.repeat(np.asarray(b), m, axis=0)


def expected_for(oracle, g2, b, ks):
    """[n, width]: [ks[i] mod r] b[i] from the oracle, one base per scalar; zero rows for an infinity base or a scalar that is 0 modulo r"""
    b = np.asarray(b, dtype=np.uint8)
    out = np.zeros_like(b)
    live = [i for i, k in enumerate(ks) if k % R and b[i].any()]
    if live:
        mul = oracle.g2_scalar_mul if g2 else oracle.g1_scalar_mul
        out[live] = np.asarray(mul(b[live].reshape(-1), rows([ks[i] % R for i in live]), threads=8)).reshape(len(live), -1)
    return out


def expected(oracle, g2, nbase, m, seed=0):
    key = (g2, nbase, m, seed)
    if key not in _expected:
        _expected[key] = expected_for(oracle, g2, expand(bases(oracle, g2, nbase), m), scalars(nbase, m, seed))
        _expected[key].setflags(write=False)
    return _expected[key]
