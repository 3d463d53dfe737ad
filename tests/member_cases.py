"""Cases of the membership tests (tests/test_membership.py on the CPU harness, tests/test_membership_gpu.py on the device): in-memory
G1, G2 and GT structs built from the big-integer oracle alone, one class per way an element can fail to be a group element, every case
with the oracle's answer.  The truth never comes from the code under test:

    every group   a coordinate whose stored 256-bit value is not below p: 0
    G1            o.g1_is_on_curve
    G2            o.g2_is_on_curve (on the twist), o.g2_in_subgroup ([r]Q = infinity by plain double-and-add)
    GT            z != 0 and o.f12_pow(z, o.R) == one  (r divides p^4 - p^2 + 1, so this implies the cyclotomic condition)

Each corpus is built once per process (seconds) and asserts that every listed class is present with the truth value it is listed for, so
no class can quietly be empty or mean something else."""
import functools
import random
from collections import Counter

import numpy as np

import bn254_py as o
import wire_cases as wc

P = o.P
MAX256 = (1 << 256) - 1


def _le(v):
    return v.to_bytes(32, "little")


def stored(b):
    """the 256-bit values a struct holds, one per coordinate"""
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def canonical(b):
    return all(v < P for v in stored(b))


def with_stored(b, slot, value):
    """the struct with the stored value of one coordinate replaced (the raw 256 bits, not a field element)"""
    return b[:32 * slot] + _le(value) + b[32 * slot + 32:]


def not_canonical_variants(b, slots):
    """p, 2^256 - 1 and (where it fits 256 bits) the coordinate's own value plus p — the same residue, so that only the range check
    can tell — in each of `slots`"""
    out = []
    for s in slots:
        own = stored(b)[s]
        for v in (P, MAX256) + ((own + P,) if own + P <= MAX256 else ()):
            out.append(with_stored(b, s, v))
    return out


class Corpus:
    """data (m, width) uint8, cls [m], truth {name: (m,) uint8}"""

    def __init__(self, width, cases, truths):
        self.width = width
        self.cls = [c for c, _ in cases]
        self.data = np.frombuffer(b"".join(b for _, b in cases), dtype=np.uint8).reshape(len(cases), width).copy()
        self.truth = {k: np.array(v, dtype=np.uint8) for k, v in truths.items()}

    def __len__(self):
        return len(self.cls)

    def counts(self):
        return Counter(self.cls)

    def of(self, cls):
        return [i for i, c in enumerate(self.cls) if c == cls]

    def check(self, expected, truth):
        """every class of `expected` {class: truth value, or None where it is decided case by case} is present and has that value"""
        n = self.counts()
        assert set(n) == set(expected), (sorted(n), sorted(expected))
        for cls, want in expected.items():
            assert n[cls] >= 1, cls
            if want is not None:
                assert all(self.truth[truth][i] == want for i in self.of(cls)), (truth, cls)

    def describe(self, i):
        return "%s[case %d]" % (self.cls[i], i)


# ------------------------------------------------------------------------------------------------ G1
G1_CLASSES = {"generator_multiple": 1, "negated": 1, "infinity": 1, "y_plus_one": 0, "swapped": 0, "coordinate_p": 0, "coordinate_max": 0,
              "coordinate_plus_p": 0}


@functools.lru_cache(maxsize=None)
def g1_cases():
    rnd = random.Random("member_cases/g1")
    pts = [o.G1_GEN, o.g1_mul(o.G1_GEN, 2), o.g1_mul(o.G1_GEN, o.R - 1)] + [o.g1_mul(o.G1_GEN, rnd.randrange(1, o.R)) for _ in range(5)]
    cases = [("generator_multiple", o.g1_to_bytes(pt)) for pt in pts]
    cases += [("negated", o.g1_to_bytes((x, (-y) % P))) for x, y in pts[:4]]
    cases.append(("infinity", bytes(64)))
    cases += [("y_plus_one", o.g1_to_bytes((x, (y + 1) % P))) for x, y in pts[:4]]
    cases += [("swapped", o.g1_to_bytes((y, x))) for x, y in pts[:4]]
    for pt in pts[:2] + [None]:
        b = o.g1_to_bytes(pt)
        for s in (0, 1):
            cases.append(("coordinate_p", with_stored(b, s, P)))
            cases.append(("coordinate_max", with_stored(b, s, MAX256)))
            if pt is not None and stored(b)[s] + P <= MAX256:
                cases.append(("coordinate_plus_p", with_stored(b, s, stored(b)[s] + P)))
    truth = [int(canonical(b) and o.g1_is_on_curve(o.g1_from_bytes(b))) for _, b in cases]
    c = Corpus(64, cases, {"on_curve": truth})
    c.check(G1_CLASSES, "on_curve")
    return c


# ------------------------------------------------------------------------------------------------ G2
# class -> (on the twist, in the subgroup)
G2_CLASSES = {"subgroup": (1, 1), "generator_multiple": (1, 1), "infinity": (1, 1), "off_subgroup": (1, 0), "cofactor_group": (1, 0), "order_10069": (1, 0),
              "subgroup_plus_cofactor": (1, 0), "y2_in_fp": (1, None), "off_twist": (0, 0), "coordinate_not_canonical": (0, 0)}


@functools.lru_cache(maxsize=None)
def g2_cases():
    pts = wc._points("g2")                                             # the point classes of the unmarshal tests, from the same oracle
    cases = []
    for cls in ("subgroup", "generator_multiple", "off_subgroup", "cofactor_group", "order_10069", "subgroup_plus_cofactor", "y2_in_fp"):
        cases += [(cls, o.g2_to_bytes(pt)) for pt in pts[cls]]
    cases.append(("infinity", bytes(128)))
    for i, (x, y) in enumerate(pts["subgroup"][:4] + pts["off_subgroup"][:2]):
        moved = [x[0], x[1], y[0], y[1]]
        moved[i % 4] = (moved[i % 4] + 1) % P
        cases.append(("off_twist", o.g2_to_bytes(((moved[0], moved[1]), (moved[2], moved[3])))))
    for pt in pts["subgroup"][:2]:
        cases += [("coordinate_not_canonical", b) for b in not_canonical_variants(o.g2_to_bytes(pt), range(4))]
    cases += [("coordinate_not_canonical", with_stored(bytes(128), s, v)) for s in range(4) for v in (P, MAX256)]
    on, sub, seen = [], [], {}
    for _, b in cases:
        if b not in seen:
            pt = o.g2_from_bytes(b) if canonical(b) else None
            seen[b] = (int(canonical(b) and o.g2_is_on_curve(pt)), int(canonical(b) and o.g2_in_subgroup(pt)))
        on.append(seen[b][0])
        sub.append(seen[b][1])
    c = Corpus(128, cases, {"on_curve": on, "in_subgroup": sub})
    c.check({k: v[0] for k, v in G2_CLASSES.items()}, "on_curve")
    c.check({k: v[1] for k, v in G2_CLASSES.items()}, "in_subgroup")
    return c


# ------------------------------------------------------------------------------------------------ GT
GT_CLASSES = {"one": 1, "pairing": 1, "pairing_power": 1, "pairing_inverse": 1, "pairing_conjugate": 1, "easy_part_only": 0, "pairing_times_easy": 0,
              "random": 0, "miller": 0, "minus_one": 0, "minus_pairing": 0, "zero": 0, "coordinate_p": 0, "coordinate_max": 0, "coordinate_plus_p": 0,
              "one_limb_changed": 0}
F12_ZERO = (o.F6_ZERO, o.F6_ZERO)


def _rand_f12(rnd):
    return tuple(tuple((rnd.randrange(P), rnd.randrange(P)) for _ in range(3)) for _ in range(2))


def is_cyclotomic(z):
    """z^(p^4) z == z^(p^2), by the oracle's coefficient-wise Frobenius"""
    return o.f12_mul(o.f12_frobenius(z, 4), z) == o.f12_frobenius(z, 2)


def easy_part(f):
    """f^((p^6 - 1)(p^2 + 1)): in the cyclotomic subgroup, of order r only by accident"""
    t = o.f12_mul(o.f12_conj(f), o.f12_inv(f))
    return o.f12_mul(o.f12_frobenius(t, 2), t)


def gt_truth(b):
    if not canonical(b):
        return 0
    z = o.gt_from_bytes(b)
    return int(z != F12_ZERO and o.f12_pow(z, o.R) == o.F12_ONE)


@functools.lru_cache(maxsize=None)
def gt_cases():
    rnd = random.Random("member_cases/gt")
    assert o.R == o.P - 6 * o.U * o.U                                  # why z^p == z^(6u^2) is z^r == 1
    pairs = [o.pair([o.g1_mul(o.G1_GEN, rnd.randrange(1, o.R))], [o.g2_mul(o.G2_GEN, rnd.randrange(1, o.R))]) for _ in range(2)]
    pairs.append(o.final_exp(_rand_f12(rnd)))                          # (a GT element without a Miller loop)
    easy = [easy_part(_rand_f12(rnd)) for _ in range(3)]
    minus_one = (((P - 1, 0), o.F2_ZERO, o.F2_ZERO), o.F6_ZERO)
    vals = [("one", o.F12_ONE)]
    vals += [("pairing", e) for e in pairs]
    vals += [("pairing_power", o.f12_pow(e, k)) for e, k in zip(pairs, (2, o.R - 1, rnd.randrange(o.R)))]
    vals += [("pairing_inverse", o.f12_inv(e)) for e in pairs[:2]]
    vals += [("pairing_conjugate", o.f12_conj(e)) for e in pairs[:2]]
    vals += [("easy_part_only", c) for c in easy]
    vals.append(("pairing_times_easy", o.f12_mul(pairs[0], easy[0])))
    vals += [("random", _rand_f12(rnd)) for _ in range(3)]
    vals.append(("miller", o.miller_loop(o.g1_mul(o.G1_GEN, 5), o.g2_mul(o.G2_GEN, 7))))
    vals.append(("minus_one", minus_one))
    vals.append(("minus_pairing", o.f12_mul(minus_one, pairs[1])))
    vals.append(("zero", F12_ZERO))
    assert all(is_cyclotomic(c) for c in easy)
    cases = [(cls, o.gt_to_bytes(z)) for cls, z in vals]
    good = o.gt_to_bytes(pairs[0])
    for s in (0, 5, 6, 11):                                            # the first and the last coordinate of each lane's half
        cases.append(("coordinate_p", with_stored(good, s, P)))
        cases.append(("coordinate_max", with_stored(good, s, MAX256)))
        if stored(good)[s] + P <= MAX256:
            cases.append(("coordinate_plus_p", with_stored(good, s, stored(good)[s] + P)))
    cases.append(("coordinate_p", with_stored(o.gt_to_bytes(F12_ZERO), 3, P)))
    for s, limb in ((0, 0), (4, 1), (7, 2), (11, 0)):                  # one 64-bit limb of one coordinate, the value still below p
        v = stored(good)[s] ^ (1 << (64 * limb + 17))
        assert v < P
        cases.append(("one_limb_changed", with_stored(good, s, v)))
    assert any(c == "coordinate_plus_p" for c, _ in cases)
    c = Corpus(384, cases, {"in_subgroup": [gt_truth(b) for _, b in cases]})
    c.check(GT_CLASSES, "in_subgroup")
    # the class that catches a missing order-r test: cyclotomic, yet not of order r
    for i in c.of("easy_part_only") + c.of("pairing_times_easy"):
        assert is_cyclotomic(o.gt_from_bytes(bytes(c.data[i]))) and not c.truth["in_subgroup"][i]
    for cls in ("random", "miller", "minus_one", "minus_pairing"):
        assert not any(is_cyclotomic(o.gt_from_bytes(bytes(c.data[i]))) for i in c.of(cls)), cls
    return c


# ------------------------------------------------------------------------------------------------ rows of a call
def tiled(corpus, n, truth, pattern="mixed"):
    """(data [n, width], want [n], idx [n]) for a call of n rows:
        mixed      a seeded permutation of all cases, repeated: good and bad elements inside every wavefront
        one_bad    good elements with ONE bad one, at a place that differs from block to block of `block` rows
        one_good   bad elements with ONE good one
        all_bad    bad elements only (a wavefront in which no element is a candidate)
    with `block` the elements of a wavefront (64 points, 32 GT elements)."""
    t = corpus.truth[truth]
    good, bad = np.nonzero(t == 1)[0], np.nonzero(t == 0)[0]
    assert len(good) and len(bad)
    rng = np.random.default_rng([254, len(corpus), n])
    if pattern == "mixed":
        idx = np.resize(rng.permutation(len(corpus)), n)
    elif pattern == "all_bad":
        idx = np.resize(rng.permutation(bad), n)
    elif pattern in ("one_bad", "one_good"):
        block = 32 if corpus.width == 384 else 64
        many, few = (good, bad) if pattern == "one_bad" else (bad, good)
        idx = np.resize(rng.permutation(many), n)
        for k, lo in enumerate(range(0, n, block)):
            idx[min(lo + (7 * k + 3) % block, n - 1)] = few[k % len(few)]
    else:
        raise ValueError(pattern)
    return np.ascontiguousarray(corpus.data[idx]), t[idx].copy(), idx
