"""One corpus of Fp12 element classes for the entries that take GT bytes without requiring them to lie in GT (gt_exp, gt_mul, gt_div,
gt_inverse, gt_multi_exp, GTFixedBase, final_exp), shared by tests/test_gt_classes.py (the host interval build) and
tests/test_gt_classes_gpu.py (the device).  Everything is Python integers over oracle/bn254_py.py; nothing comes from the code under test.

The kernels choose their path by two predicates, and the classes are the combinations of their answers:

    cyclotomic   z^(p^4) z == z^(p^2)       Granger-Scott squarings in f12p_exp256, wide_exp256, f12p_multi_exp
    norm one     C0^2 - v C1^2 == 1 in Fp6  (z conj(z) == 1, z^(p^6 + 1) == 1): the conjugate as the inverse in f12_inv_gt

    class                                    cyclotomic  norm one
    one, pairing, pairing_inverse            yes         yes         of order r
    cyclotomic_not_gt                        yes         yes         easy_part(random): z^r != 1
    norm_one_only                            NO          yes         conj(f) / f, the first step of the easy part alone
    minus_one, minus_pairing                 no          yes         (-1)^(p^4 - p^2 + 1) = -1
    miller, random                           no          no
    in_fp, in_fp2, in_fp6 (C1 = 0),          no          no          the easy part of the final exponentiation gives exactly one
    pure_w (C0 = 0)
    single_coordinate                        no          no          one of the twelve Fp coordinates 1 or p - 1, the rest zero
    zero                                     -           -           0^k = 0 for k > 0, 0^0 = 1, 1 / 0 = 0

Cyclotomic implies norm one (p^4 - p^2 + 1 divides p^6 + 1); `norm_one_only` is the class that tells a cyclotomic test from a norm-one
test, and the module asserts at import that it is there with (cyclotomic, norm one) = (no, yes).  Every class has at least two
members, except one, minus_one and zero, which are single elements.  single_coordinate sits at the coordinates 0, 5, 6 and 11 (the first
and the last of each lane's half); at coordinate 0 the two values ARE one and minus_one, which is asserted, and they stand in their own
classes.  Zero satisfies the cyclotomic equation as the kernels read it (0 * 0 == 0) and has norm zero: its truths are recorded as the
predicates' answers, the table claims nothing for it.

Expectations are one big-integer statement each, cached per (element, argument): f12_pow with the exponent as it is (never reduced
modulo r), f12_inv with 1 / 0 = 0, final_exp_direct (ONE power by s (p^12 - 1) / r, independent of the easy / hard split).

Layouts put one foreign element into an array of a background class at the places where a per-wavefront vote can go wrong: lane 0 of
a wavefront, its last lane, and alone in the partial last wavefront, for wavefronts of 32 elements (the lane-pair forms) and of 64 (one
element per lane)."""
import functools
import random

import numpy as np

import bn254_py as o
from member_cases import F12_ZERO, _rand_f12, easy_part, is_cyclotomic

P, R = o.P, o.R
GT = 384
MINUS_ONE = (((P - 1, 0), o.F2_ZERO, o.F2_ZERO), o.F6_ZERO)

# class -> (cyclotomic, norm one); None: not claimed
CLASSES = {"one": (1, 1), "pairing": (1, 1), "pairing_inverse": (1, 1), "cyclotomic_not_gt": (1, 1), "norm_one_only": (0, 1), "minus_one": (0, 1),
           "minus_pairing": (0, 1), "miller": (0, 0), "random": (0, 0), "in_fp": (0, 0), "in_fp2": (0, 0), "in_fp6": (0, 0), "pure_w": (0, 0),
           "single_coordinate": (0, 0), "zero": (None, None)}
ORDER_R = ("one", "pairing", "pairing_inverse")
SINGLETONS = ("one", "minus_one", "zero")
EASY_PART_ONE = ("in_fp", "in_fp2", "in_fp6", "pure_w")               # final_exp gives exactly one
COORDINATES = (0, 5, 6, 11)

_rnd = random.Random("f12_cases/exponents")
EXPONENTS = [0, 1, 2, R - 1, R, R + 1, 1 << 255, (1 << 256) - 1, _rnd.getrandbits(256) | 1 << 255, _rnd.getrandbits(256)]
SIZES = (1, 31, 32, 33, 63, 64, 65, 130)
WAVE_ELEMENTS = (32, 64)                                               # one element per lane pair, one per lane
# (background, foreigner): each foreigner alone in its array
COMBINATIONS = (("pairing", "norm_one_only"), ("pairing", "minus_pairing"), ("pairing", "cyclotomic_not_gt"), ("pairing", "zero"), ("norm_one_only", "pairing"))


def has_norm_one(z):
    return o.f6_sub(o.f6_mul(z[0], z[0]), o.f6_mul_v(o.f6_mul(z[1], z[1]))) == o.F6_ONE


def f12_neg(z):
    return (o.f6_neg(z[0]), o.f6_neg(z[1]))


def _coordinate(slot, value):
    c = [0] * 12
    c[slot] = value
    f2 = [(c[2 * i], c[2 * i + 1]) for i in range(6)]
    return (tuple(f2[:3]), tuple(f2[3:]))


def to_row(z):
    return np.frombuffer(o.gt_to_bytes(z), dtype=np.uint8)


class F12Corpus:
    """cls [m], val [m] (Python tuples), rows (m, 384) uint8 in gnark's in-memory form, cyclotomic / norm_one (m,) uint8"""

    def __init__(self, members):
        self.cls = [c for c, _ in members]
        self.val = [z for _, z in members]
        self.rows = np.stack([to_row(z) for z in self.val])
        self.cyclotomic = np.array([int(is_cyclotomic(z)) for z in self.val], dtype=np.uint8)
        self.norm_one = np.array([int(has_norm_one(z)) for z in self.val], dtype=np.uint8)

    def __len__(self):
        return len(self.cls)

    def of(self, cls):
        return [i for i, c in enumerate(self.cls) if c == cls]

    def describe(self, i):
        return "%s[element %d]" % (self.cls[i], i)


@functools.lru_cache(maxsize=None)
def corpus():
    rnd = random.Random("f12_cases/corpus")
    fp = lambda: rnd.randrange(2, P - 1)
    f2 = lambda: (fp(), fp())
    pairs = [o.pair([o.g1_mul(o.G1_GEN, rnd.randrange(1, R))], [o.g2_mul(o.G2_GEN, rnd.randrange(1, R))]) for _ in range(2)]
    m = [("one", o.F12_ONE)]
    m += [("pairing", e) for e in pairs]
    m += [("pairing_inverse", o.f12_inv(e)) for e in pairs]
    m += [("cyclotomic_not_gt", easy_part(_rand_f12(rnd))) for _ in range(2)]
    for _ in range(2):
        f = _rand_f12(rnd)
        m.append(("norm_one_only", o.f12_mul(o.f12_conj(f), o.f12_inv(f))))
    m.append(("minus_one", MINUS_ONE))
    m += [("minus_pairing", f12_neg(e)) for e in pairs]
    m += [("miller", o.miller_loop(o.g1_mul(o.G1_GEN, a), o.g2_mul(o.G2_GEN, b))) for a, b in ((5, 7), (rnd.randrange(1, R), rnd.randrange(1, R)))]
    m += [("random", _rand_f12(rnd)) for _ in range(2)]
    m += [("in_fp", (((a, 0), o.F2_ZERO, o.F2_ZERO), o.F6_ZERO)) for a in (2, fp())]
    m += [("in_fp2", ((f2(), o.F2_ZERO, o.F2_ZERO), o.F6_ZERO)) for _ in range(2)]
    m += [("in_fp6", ((f2(), f2(), f2()), o.F6_ZERO)) for _ in range(2)]
    m += [("pure_w", (o.F6_ZERO, (f2(), f2(), f2()))) for _ in range(2)]
    assert _coordinate(0, 1) == o.F12_ONE and _coordinate(0, P - 1) == MINUS_ONE       # coordinate 0: the classes of those names
    m += [("single_coordinate", _coordinate(s, v)) for s in COORDINATES[1:] for v in (1, P - 1)]
    m.append(("zero", F12_ZERO))
    c = F12Corpus(m)
    # the corpus asserts its own truths
    assert set(c.cls) == set(CLASSES) and len(set(c.rows.tobytes()[GT * i:GT * i + GT] for i in range(len(c)))) == len(c)
    for cls, (cyc, n1) in CLASSES.items():
        assert len(c.of(cls)) >= (1 if cls in SINGLETONS else 2), cls
        for i in c.of(cls):
            assert cyc is None or c.cyclotomic[i] == cyc, (cls, "cyclotomic")
            assert n1 is None or c.norm_one[i] == n1, (cls, "norm one")
            if cls != "zero":
                assert (o.f12_pow(c.val[i], R) == o.F12_ONE) == (cls in ORDER_R), (cls, "order r")
    assert all(c.norm_one[i] for i in range(len(c)) if c.cyclotomic[i] and c.cls[i] != "zero")
    assert any(not c.cyclotomic[i] and c.norm_one[i] for i in c.of("norm_one_only"))    # the discriminating element is there
    assert c.cyclotomic[c.of("zero")[0]] == 1 and c.norm_one[c.of("zero")[0]] == 0     # what the predicates answer for zero
    for i in range(len(c)):
        assert o.gt_from_bytes(c.rows[i].tobytes()) == c.val[i]
    return c


# ------------------------------------------------------------------------------------------------ expectations (i: an index of the corpus)
@functools.lru_cache(maxsize=None)
def power(i, k):
    """x_i^k as a value, k as the integer it is"""
    z = corpus().val[i]
    if z == F12_ZERO:
        return o.F12_ONE if k == 0 else F12_ZERO
    return o.f12_pow(z, k)


@functools.lru_cache(maxsize=None)
def inverse(i):
    z = corpus().val[i]
    return F12_ZERO if z == F12_ZERO else o.f12_inv(z)


@functools.lru_cache(maxsize=None)
def final_exp(i):
    z = corpus().val[i]
    return F12_ZERO if z == F12_ZERO else o.final_exp_direct(z)


def rows_of(values):
    values = list(values)
    return np.stack([to_row(z) for z in values]) if values else np.zeros((0, GT), dtype=np.uint8)


def exponent_rows(ks):
    return np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in ks), dtype=np.uint8).reshape(-1, 32).copy()


def exponents_of(i):
    """the exponents element i is raised to: all of EXPONENTS for the first member of a class; r, 2^256 - 1, a random one and 2 for the
    others (every power is a 256-step big-integer loop: the list keeps the expectations of a whole module to a few seconds)"""
    c = corpus()
    return EXPONENTS if i == c.of(c.cls[i])[0] else [R, (1 << 256) - 1, EXPONENTS[-1], 2]


def exponents_for(idx, shift=0):
    """one exponent per position from the element's list, so that the foreigner of a layout meets a different one from layout to layout"""
    return [exponents_of(int(i))[(3 * j + shift) % len(exponents_of(int(i)))] for j, i in enumerate(idx)]


def want_exp(idx, ks):
    return rows_of(power(int(i), int(k)) for i, k in zip(idx, ks))


def want_inverse(idx):
    return rows_of(inverse(int(i)) for i in idx)


def want_final_exp(idx):
    return rows_of(final_exp(int(i)) for i in idx)


def want_mul(a_idx, b_idx):
    c = corpus()
    return rows_of(o.f12_mul(c.val[int(a)], c.val[int(b)]) for a, b in zip(a_idx, b_idx))


def want_div(a_idx, b_idx):
    c = corpus()
    return rows_of(o.f12_mul(c.val[int(a)], inverse(int(b))) for a, b in zip(a_idx, b_idx))


def want_multi_exp(idx, ks, seg):
    out = []
    for s in range(len(seg) - 1):
        acc = o.F12_ONE
        for j in range(seg[s], seg[s + 1]):
            acc = o.f12_mul(acc, power(int(idx[j]), int(ks[j])))
        out.append(acc)
    return rows_of(out)


def class_exponent_cases():
    """(idx, ks): every element under every exponent of its list (exponents_of), class by class, the first member first"""
    c = corpus()
    idx, ks = [], []
    for cls in CLASSES:
        for i in c.of(cls):
            for k in exponents_of(i):
                idx.append(i)
                ks.append(k)
    return np.array(idx), ks


def multi_exp_case(per_wave):
    """(idx, ks, seg) of a segmented multi-exponentiation in segments of four factors, the group that shares one squaring chain and one
    vote; a segment of four is one piece, so `per_wave` consecutive segments are the lane pairs of one wavefront (32 on the device; 1
    where the pair is the wavefront).  In order: a wavefront of cyclotomic groups; one of cyclotomic groups with a group of norm_one_only
    and the four groups that hold one norm_one_only among three pairing values, at each place; a wavefront of norm_one_only groups; then
    every element of the corpus four at a time.  The exponents run through EXPONENTS, r and 2^256 - 1 among them."""
    c = corpus()
    cyc = c.of("pairing") + c.of("pairing_inverse") + c.of("cyclotomic_not_gt")
    noo = c.of("norm_one_only")
    groups = [[cyc[(4 * s + t) % len(cyc)] for t in range(4)] for s in range(per_wave)]
    mixed = [[cyc[(s + t) % len(cyc)] for t in range(4)] for s in range(per_wave)]
    special = [[noo[t % 2] for t in range(4)]] + [[noo[p % 2] if t == p else cyc[t] for t in range(4)] for p in range(4)]
    if per_wave > 1:
        assert per_wave >= 32
        for j, g in enumerate(special):
            mixed[(7 * j + 3) % per_wave] = g                          # lane pairs 3, 10, 17, 24 and 31 of that wavefront
        groups += mixed
    else:
        groups += special
    groups += [[noo[(s + t) % 2] for t in range(4)] for s in range(per_wave)]
    groups += [[(4 * s + t) % len(c) for t in range(4)] for s in range(-(-len(c) // 4))]
    idx = np.array([i for g in groups for i in g])
    ks = [exponents_of(int(i))[(7 * j + j // 10) % len(exponents_of(int(i)))] for j, i in enumerate(idx)]
    return idx, ks, list(range(0, len(idx) + 1, 4))


# ------------------------------------------------------------------------------------------------ layouts
def foreign_positions(n):
    """the places of a lone foreigner in an array of n: lane 0 of the last wavefront and of a middle one, the last lane of the first
    wavefront, and (n = 1 modulo the wavefront) alone in the partial last wavefront — for wavefronts of 32 and of 64 elements"""
    at = set()
    for B in WAVE_ELEMENTS:
        waves = -(-n // B)
        at.add(B * (waves - 1))                                        # lane 0 of the last wavefront; alone in it when n % B == 1
        if waves >= 3:
            at.add(B)                                                  # lane 0 of a wavefront with full neighbours on both sides
        at.add(min(B, n) - 1)                                          # the last lane of the first wavefront
    return sorted(at)


@functools.lru_cache(maxsize=None)
def layouts():
    """[(label, idx)]: idx (n,) indices of the corpus.  The background alternates between the members of its class."""
    c = corpus()
    out = []
    for n in SIZES:
        for bg, fg in COMBINATIONS:
            b, f = c.of(bg), c.of(fg)
            for t, pos in enumerate(foreign_positions(n)):
                idx = np.array([b[j % len(b)] for j in range(n)], dtype=np.int64)
                idx[pos] = f[(t + n) % len(f)]
                out.append(("%s with %s at %d of %d" % (bg, fg, pos, n), idx))
        out.append(("every class in turn, %d" % n, (np.arange(n) + n) % len(c)))
    return out


def wave_mix(idx, B):
    """per wavefront of B elements: the set of (cyclotomic, norm one) answers in it"""
    c = corpus()
    return [set(zip(c.cyclotomic[idx[lo:lo + B]].tolist(), c.norm_one[idx[lo:lo + B]].tolist())) for lo in range(0, len(idx), B)]


def _check_layouts():
    """both wavefront sizes see, inside ONE array, a full uniform wavefront and a mixed one; and the three places are all taken"""
    lone = [(l, i) for l, i in layouts() if " with " in l]
    for B in WAVE_ELEMENTS:
        assert any(any(len(s) == 1 for s in wave_mix(i, B)[:len(i) // B]) and any(len(s) > 1 for s in wave_mix(i, B)) for _, i in lone), B
        for place in (lambda i, p: p % B == 0 and p > 0, lambda i, p: p % B == B - 1, lambda i, p: p % B == 0 and p == len(i) - 1 and p > 0):
            assert any(place(i, int(l.split(" at ")[1].split(" of ")[0])) for l, i in lone), B


_check_layouts()
