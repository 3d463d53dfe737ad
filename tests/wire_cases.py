"""Cases of the unmarshal / marshal / map-to-curve edge tests (tests/test_wire.py and tests/test_hash_to_curve.py on the CPU harness,
tests/test_decode_forms_gpu.py on the device): encodings and pairs of field elements built from the big-integer oracle alone, one
class per way a decoder or the map can go wrong, every case with the oracle's answer (ok and the memory row, all zero where ok = 0).
Expectations are computed once per unique case; tiled() repeats the cases to the size of a call in two arrangements.  Each corpus
is built once per process (seconds) and checks its own class minimums, so no search loop below can quietly return an empty class."""
import functools
import random
from collections import Counter, namedtuple

import numpy as np

import bn254_py as o
from conftest import load_golden

P = o.P
Case = namedtuple("Case", "data cls ok row")            # input bytes, class name, expected ok (0 / 1), expected output row


class Corpus:
    """cases plus their columns as arrays: data (m, width in), ok (m,), rows (m, width out)"""

    def __init__(self, cases):
        self.cases = cases
        self.cls = [c.cls for c in cases]
        self.data = np.frombuffer(b"".join(c.data for c in cases), dtype=np.uint8).reshape(len(cases), -1).copy()
        self.ok = np.array([c.ok for c in cases], dtype=np.uint8)
        self.rows = np.frombuffer(b"".join(c.row for c in cases), dtype=np.uint8).reshape(len(cases), -1).copy()

    def __len__(self):
        return len(self.cases)

    def counts(self):
        return Counter(self.cls)

    def describe(self, i):
        """what an assertion message says about case i"""
        return "%s[case %d, ok %d]" % (self.cls[i], i, self.ok[i])


def tiled(corpus, n, arrangement):
    """n rows of the corpus: (data, ok, rows, idx) with idx[j] = the case at row j.  "shuffled": a seeded permutation of the cases,
    repeated, so that every wavefront mixes accept, refuse, infinity and compressed rows.  "runs": sorted by class, every class
    filling blocks of 64 rows (a whole wavefront of the one-element-per-lane kernels, 4 / 8 of the quad / octet kernels) with its
    cases in turn, the sequence of blocks repeated, so that whole wavefronts take one path."""
    m = len(corpus)
    if arrangement == "shuffled":
        idx = np.resize(np.random.default_rng([254, m, n]).permutation(m), n)
    elif arrangement == "runs":
        by_cls = {}
        for i, c in enumerate(corpus.cls):
            by_cls.setdefault(c, []).append(i)
        idx = np.resize(np.concatenate([np.resize(np.array(ids), 64 * -(-len(ids) // 64)) for _, ids in sorted(by_cls.items())]), n)
    else:
        raise ValueError(arrangement)
    return np.ascontiguousarray(corpus.data[idx]), corpus.ok[idx].copy(), np.ascontiguousarray(corpus.rows[idx]), idx


ARRANGEMENTS = ("shuffled", "runs")


def mismatches(corpus, idx, got_rows, got_ok, want_rows, want_ok):
    """rows of a call that differ from the expectation, as text that names class, case and row position ("" when none)"""
    got_rows, got_ok = np.asarray(got_rows), np.asarray(got_ok).reshape(-1)
    bad = np.nonzero((got_rows.reshape(want_rows.shape) != want_rows).any(axis=1) | (got_ok != want_ok))[0]
    if bad.size == 0:
        return ""
    return "%d of %d rows wrong; first: %s" % (bad.size, len(idx), ", ".join(
        "row %d (%d mod 64) %s got ok %d" % (j, j % 64, corpus.describe(idx[j]), got_ok[j]) for j in bad[:6]))


# ------------------------------------------------------------------------------------------------ number theory the oracle lacks
def fp_cbrt(a):
    """A cube root of a in Fp or None.  p = 1 (mod 9): write p - 1 = 3^s t; a^e with 3 e = 1 + k t is a root up to an element of
    the 3-Sylow subgroup, whose logarithm to the base of a generator g is found digit by digit (Pohlig-Hellman, as Tonelli-Shanks
    does for exponent 2)."""
    a %= P
    if a == 0:
        return 0
    if pow(a, (P - 1) // 3, P) != 1:
        return None
    s, t = 0, P - 1
    while t % 3 == 0:
        s, t = s + 1, t // 3
    c = 2
    while pow(c, (P - 1) // 3, P) == 1:
        c += 1
    g = pow(c, t, P)                                                  # generates the 3-Sylow subgroup (order 3^s)
    e = pow(3, -1, t)
    k = (3 * e - 1) // t
    b, g3 = pow(a, t, P), pow(g, 3, P)                                # b = g3^m: a is a cube
    w = pow(g3, 3 ** (s - 2), P) if s >= 2 else 1                     # of order 3
    m = 0
    for i in range(s - 1):
        d = pow(b * pow(g3, -m, P) % P, 3 ** (s - 2 - i), P)
        digit = 0 if d == 1 else 1 if d == w else 2
        assert digit < 2 or d == w * w % P
        m += digit * 3 ** i
    r = pow(a, e, P) * pow(g, -m * k, P) % P
    assert pow(r, 3, P) == a
    return r


@functools.lru_cache(maxsize=None)
def lex_boundary_points():
    """G1 points with y within 2^32 of (p - 1) / 2: ([y <= (p-1)/2 ...], [y >= (p+1)/2 ...]).  wire_words_lex_largest decides them in
    its lowest word only.  The two sides are the two signs of the same points."""
    half = (P - 1) // 2
    lo, hi = [], []
    for j in range(64):
        for y, side in ((half - j, lo), (half + 1 + j, hi)):
            x = fp_cbrt(y * y - o.B_G1)
            if x is not None:
                assert o.g1_is_on_curve((x, y))
                side.append((x, y))
        if len(lo) >= 3 and len(hi) >= 3:
            break
    assert len(lo) >= 2 and len(hi) >= 2, (len(lo), len(hi))
    assert all(not o.fp_lex_largest(p[1]) for p in lo) and all(o.fp_lex_largest(p[1]) for p in hi)
    return lo, hi


def _g2_rhs(x):
    return o.f2_add(o.f2_mul(o.f2_sqr(x), x), o.B_G2)


@functools.lru_cache(maxsize=None)
def twist_points_y2_in_fp():
    """Twist points (x, y, kind) whose y^2 lies in Fp: x = (a, b) with a^2 = (b^3 - Im b') / (3 b), b = 3, 4, ...; kind is "real"
    where y = (r, 0) and "imag" where y = (0, r).  f2_sqrt takes its "a lies in Fp" branch on them, f2_lex_largest its a1 == 0 path
    (real) and sgn0 its a0 == 0 path (imag).  None lies in the order-r subgroup."""
    out, b = [], 3
    while len(out) < 8 or sum(k == "real" for _, _, k in out) < 2 or sum(k == "imag" for _, _, k in out) < 2:
        assert b < 200
        a = o.fp_sqrt((b ** 3 - o.B_G2[1]) * pow(3 * b, -1, P) % P)
        if a is not None:
            x = (a, b)
            y2 = _g2_rhs(x)
            assert y2[1] == 0
            y = o.f2_sqrt(y2)
            assert y is not None and (y[0] == 0) != (y[1] == 0) and o.g2_is_on_curve((x, y))
            out.append((x, y, "real" if y[1] == 0 else "imag"))
        b += 1
    assert not any(o.g2_in_subgroup((x, y)) for x, y, _ in out)
    return out


def word_boundary_values():
    """[(name, value, canonical)]: for every 32-bit word k of p the value that agrees with p above word k, is one less in word k and all
    ones below (canonical), and the one that is one more in word k and zero below (not canonical); then p - 1 and p.  A comparison
    that goes word by word from the top decides each of the first sixteen at word k exactly."""
    out = []
    for k in range(8):
        hi = (P >> (32 * (k + 1))) << (32 * (k + 1))
        wk = (P >> (32 * k)) & 0xFFFFFFFF
        assert 0 < wk < 0xFFFFFFFF
        out.append(("below%d" % k, hi | ((wk - 1) << (32 * k)) | ((1 << (32 * k)) - 1), True))
        out.append(("above%d" % k, hi | ((wk + 1) << (32 * k)), False))
    out += [("p-1", P - 1, True), ("p", P, False)]
    assert all((v < P) == canon and v < 1 << 256 for _, v, canon in out)
    return out


# ------------------------------------------------------------------------------------------------ groups
def _be(v):
    return v.to_bytes(32, "big")


def _filler(n, salt):
    """n non-zero bytes (what follows a compressed element in a wide slot)"""
    return bytes((i * 37 + salt * 11) % 255 + 1 for i in range(n))


class _Group:
    def __init__(self, g2):
        self.g2 = g2
        self.name = "g2" if g2 else "g1"
        self.comp_w, self.raw_w = (64, 128) if g2 else (32, 64)
        self.unmarshal = o.g2_unmarshal if g2 else o.g1_unmarshal
        self.marshal = o.g2_marshal if g2 else o.g1_marshal
        self.to_bytes = o.g2_to_bytes if g2 else o.g1_to_bytes
        self.from_bytes = o.g2_from_bytes if g2 else o.g1_from_bytes
        self.neg = o.g2_neg if g2 else o.g1_neg
        self.mul = o.g2_mul if g2 else o.g1_mul
        self.gen = o.G2_GEN if g2 else o.G1_GEN

    def coords(self, pt):
        """the coordinates in wire order"""
        return [pt[0][1], pt[0][0], pt[1][1], pt[1][0]] if self.g2 else [pt[0], pt[1]]

    def x_without_root(self, rnd):
        while True:
            if self.g2:
                x = (rnd.randrange(P), rnd.randrange(P))
                if o.f2_sqrt(_g2_rhs(x)) is None:
                    return [x[1], x[0]]
            else:
                x = rnd.randrange(P)
                if o.fp_sqrt((x ** 3 + o.B_G1) % P) is None:
                    return [x]


GROUPS = {"g1": _Group(False), "g2": _Group(True)}
SLOTS = {"g1": (32, 64), "g2": (64, 128)}


def _rand_twist(rnd):
    while True:
        x = (rnd.randrange(P), rnd.randrange(P))
        y = o.f2_sqrt(_g2_rhs(x))
        if y is not None:
            return (x, y)


@functools.lru_cache(maxsize=None)
def _points(kind):
    """the points behind the decode classes of one group (shared by its two slot sizes)"""
    G = GROUPS[kind]
    rnd = random.Random("wire_cases/points/" + kind)
    pts = {"subgroup": [G.mul(G.gen, rnd.randrange(1, o.R)) for _ in range(10)],
           "generator_multiple": [G.gen, G.mul(G.gen, 2), G.mul(G.gen, o.R - 1)]}
    if kind == "g1":
        lo, hi = lex_boundary_points()
        pts["lex_boundary"] = lo + hi
    else:
        h2 = 2 * P - o.R
        assert h2 % 10069 == 0
        pts["off_subgroup"] = [_rand_twist(rnd) for _ in range(8)]
        cof = []
        while len(cof) < 4:
            t = o.g2_mul_plain(_rand_twist(rnd), o.R)                  # order divides h2
            if t is not None:
                cof.append(t)
        pts["cofactor_group"] = cof
        small = []
        while len(small) < 2:
            t = o.g2_mul_plain(_rand_twist(rnd), (h2 // 10069) * o.R)
            if t is not None:
                small.append(t)
        pts["order_10069"] = small
        pts["subgroup_plus_cofactor"] = [o.g2_add(pts["subgroup"][i], cof[i]) for i in range(4)]
        pts["y2_in_fp"] = [(x, y) for x, y, _ in twist_points_y2_in_fp()]
    return pts


# class -> (expected ok or None where the oracle decides case by case, minimum count in a wide slot, in a narrow slot)
_ACCEPT = {"subgroup": 16, "infinity": 1, "generator_multiple": 3, "lex_boundary": 8}
_REFUSE_G2 = {"off_subgroup": 8, "cofactor_group": 4, "order_10069": 2, "subgroup_plus_cofactor": 4, "y2_in_fp": 8}
_REFUSE = {"x_without_root": 4, "coordinate_not_canonical": 3, "compressed_x_not_canonical": 6, "infinity_stray_bit": 4}


@functools.lru_cache(maxsize=None)
def decode_cases(kind, slot):
    """the decode corpus of one group ("g1" / "g2") in slots of `slot` bytes.  In a wide slot a row is uncompressed, compressed (the
    rest of the slot non-zero) or infinity; in a narrow slot an uncompressed flag is the short-buffer rejection."""
    G = GROUPS[kind]
    assert slot in (G.comp_w, G.raw_w)
    wide = slot == G.raw_w
    rnd = random.Random("wire_cases/decode/%s/%d" % (kind, slot))
    pts = _points(kind)
    raw = []

    def add(cls, enc):
        assert len(enc) in (G.comp_w, G.raw_w)
        if len(enc) > slot:
            enc = enc[:slot]                                           # (an uncompressed element cut to a narrow slot: short buffer)
        raw.append((cls, enc + _filler(slot - len(enc), len(raw))))

    def flagged(words, flag):
        """compressed encoding of the x words (wire order, the first below 2^254) under a flag"""
        b = bytearray(b"".join(_be(v) for v in words))
        assert b[0] & o.M_MASK == 0
        b[0] |= flag
        return bytes(b)

    def add_point(cls, pt, both_flags):
        comp = G.marshal(pt, True)
        add(cls, comp)
        if both_flags:
            add(cls, bytes([comp[0] ^ 0x40]) + comp[1:])               # the other sign flag: the opposite point
        if wide:
            add(cls, G.marshal(pt))

    for cls in ("subgroup", "generator_multiple", "lex_boundary", "off_subgroup", "cofactor_group", "order_10069", "subgroup_plus_cofactor", "y2_in_fp"):
        for pt in pts.get(cls, ()):
            add_point(cls, pt, cls in ("subgroup", "lex_boundary", "y2_in_fp"))
    # infinity in each legal encoding (a narrow slot has one)
    add("infinity", bytes([o.M_INFINITY]) + bytes(G.comp_w - 1))
    if wide:
        add("infinity", bytes(G.raw_w))
        add("infinity", bytes([o.M_INFINITY]) + bytes(G.raw_w - 1))
    else:
        add("short_buffer", bytes(G.raw_w))
        for pt in pts["subgroup"][:3]:
            add("short_buffer", G.marshal(pt))
    # on no curve: a coordinate of a point moved by one
    if wide:
        for i, pt in enumerate(pts["subgroup"][:4]):
            c = G.coords(pt)
            c[(i + 1) % len(c)] = (c[(i + 1) % len(c)] + 1) % P
            add("not_on_curve", b"".join(_be(v) for v in c))
    for i in range(4):
        add("x_without_root", flagged(G.x_without_root(rnd), (o.M_SMALLEST, o.M_LARGEST)[i & 1]))
    # values that no coordinate may hold, in every coordinate slot
    if wide:
        for i, pt in enumerate(pts["subgroup"][:3]):
            for j in range(len(G.coords(pt))):
                for v in (P, P + 1, (1 << 256) - 1):
                    c = G.coords(pt)
                    c[j] = v
                    add("coordinate_not_canonical", b"".join(_be(v) for v in c))
    x_words = G.coords(pts["subgroup"][4])[:G.comp_w // 32]
    for j in range(len(x_words)):
        for v in (P, P + 1, (1 << 254) - 1 if j == 0 else (1 << 256) - 1):
            for flag in (o.M_SMALLEST, o.M_LARGEST):
                w = list(x_words)
                w[j] = v
                add("compressed_x_not_canonical", flagged(w, flag))
    # the infinity flag with one stray bit: first byte, last byte of the first half, first and last byte of the second half
    for pos, bit in ((0, 0x01), (0, 0x20), (G.comp_w // 2 - 1, 0x01), (G.comp_w // 2 - 1, 0x80), (G.comp_w // 2, 0x80), (G.comp_w // 2, 0x01),
                     (G.comp_w - 1, 0x01), (G.comp_w - 1, 0x80)):
        b = bytearray([o.M_INFINITY]) + bytearray(G.comp_w - 1)
        b[pos] |= bit
        add("infinity_stray_bit", bytes(b))
    # the word-boundary values in every coordinate slot: whatever the oracle answers is the expectation
    base = G.coords(G.gen)
    for name, v, canon in word_boundary_values():
        for j in range(len(base)):
            if wide:
                c = list(base)
                c[j] = v
                add("word_boundary", b"".join(_be(v) for v in c))
            if j < len(x_words) and (j > 0 or v < 1 << 254):
                w = list(base[:len(x_words)])
                w[j] = v
                add("word_boundary", flagged(w, o.M_SMALLEST))

    expect = {}
    cases = []
    for cls, enc in raw:
        if enc not in expect:
            pt, ok = G.unmarshal(enc)
            expect[enc] = (int(bool(ok)), G.to_bytes(pt if ok else None))
        cases.append(Case(enc, cls, *expect[enc]))
    corpus = Corpus(cases)
    n = corpus.counts()
    for cls, least in _ACCEPT.items():
        if cls in pts or cls == "infinity":
            assert n[cls] >= (least if not (cls == "infinity" and wide) else 2), (kind, slot, cls, n[cls])
            assert all(c.ok == 1 for c in cases if c.cls == cls), (kind, slot, cls)
    for cls, least in list(_REFUSE.items()) + (list(_REFUSE_G2.items()) if G.g2 else []) + [("not_on_curve", 4)] * wide + [("short_buffer", 2)] * (not wide):
        if cls == "coordinate_not_canonical" and not wide:
            continue
        assert n[cls] >= least, (kind, slot, cls, n[cls])
        assert all(c.ok == 0 and not any(c.row) for c in cases if c.cls == cls), (kind, slot, cls)
    if not G.g2:                                                       # (no such value is the x of a G2 subgroup point: GT separates them)
        assert {c.ok for c in cases if c.cls == "word_boundary"} == {0, 1}, (kind, slot)
    assert all(c.ok or not any(c.row) for c in cases)
    assert 3 * int((corpus.ok == 0).sum()) >= len(cases), (kind, slot, int((corpus.ok == 0).sum()), len(cases))
    return corpus


@functools.lru_cache(maxsize=None)
def gt_decode_cases():
    """GT decoding accepts any tuple of twelve canonical coefficients, so ok separates the word-boundary values cleanly: each of them,
    and 0, 1, p + 1 and 2^256 - 1, in each of the twelve slots among seeded canonical coefficients; a few whole canonical tuples."""
    rnd = random.Random("wire_cases/gt")
    vals = [(n, v) for n, v, _ in word_boundary_values()] + [("0", 0), ("1", 1), ("p+1", P + 1), ("2^256-1", (1 << 256) - 1)]
    raw = []
    for name, v in vals:
        for j in range(12):
            c = [rnd.randrange(P) for _ in range(12)]
            c[j] = v
            raw.append(("canonical_boundary_accept" if v < P else "canonical_boundary_refuse", b"".join(_be(x) for x in c)))
    raw += [("canonical_tuple", b"".join(_be(rnd.randrange(P)) for _ in range(12))) for _ in range(6)]
    raw += [("canonical_tuple", bytes(384)), ("canonical_tuple", o.gt_marshal(o.F12_ONE))]
    cases = []
    for cls, enc in raw:
        v, ok = o.gt_unmarshal(enc)
        cases.append(Case(enc, cls, int(bool(ok)), o.gt_to_bytes(v) if ok else bytes(384)))
    corpus = Corpus(cases)
    n = corpus.counts()
    assert n["canonical_boundary_accept"] == 132 and n["canonical_boundary_refuse"] == 132
    assert all(c.ok == (c.cls != "canonical_boundary_refuse") for c in cases)
    assert 3 * int((corpus.ok == 0).sum()) >= len(cases)
    return corpus


@functools.lru_cache(maxsize=None)
def marshal_cases(kind, compressed):
    """points to encode (memory rows) with the oracle's encoding as the expected row: every point the wide decode corpus accepts (infinity
    and, for G1, the lex-boundary points among them) and, for G2, both signs of the twist points whose y has a zero half — marshal
    makes no subgroup test, so these run f2_lex_largest's a1 == 0 path and its a0 == 0 path."""
    G = GROUPS[kind]
    seen, pts = set(), []
    for c in decode_cases(kind, G.raw_w).cases:
        if c.ok and c.row not in seen:
            seen.add(c.row)
            pts.append((c.cls, G.from_bytes(c.row)))
    if G.g2:
        for x, y, k in twist_points_y2_in_fp():
            pts += [("y2_in_fp_" + k, (x, y)), ("y2_in_fp_" + k, (x, o.f2_neg(y)))]
    cases = [Case(G.to_bytes(pt), cls, 1, G.marshal(pt, compressed)) for cls, pt in pts]
    n = Counter(c.cls for c in cases)
    assert n["infinity"] >= 1 and n["subgroup"] >= 16
    if G.g2:
        assert n["y2_in_fp_real"] >= 4 and n["y2_in_fp_imag"] >= 4
        if compressed:                                                 # both flags occur in each kind
            for k in ("real", "imag"):
                assert {c.row[0] & o.M_MASK for c in cases if c.cls == "y2_in_fp_" + k} == {o.M_SMALLEST, o.M_LARGEST}
    else:
        assert n["lex_boundary"] >= 4
    return Corpus(cases)


# ------------------------------------------------------------------------------------------------ map to curve
def _exceptional_us(F, consts):
    """u with 1 - c1 u^2 = 0 or 1 + c1 u^2 = 0 (tv1 tv2 = 0: inv0 returns 0), where they exist in the field"""
    c1i = F.inv0(consts[1])
    return [u for u in (F.sqrt(c1i), F.sqrt(F.neg(c1i))) if u is not None]


@functools.lru_cache(maxsize=None)
def g2_us_onto_y2_in_fp():
    """[(u, kind)]: Fp2 elements that the SVDW map sends to an x1 whose g(x1) lies in Fp (the x of twist_points_y2_in_fp): solve
    (c2 - x)(1 + c1 u^2) = c3 u for u and keep the roots that the oracle's map sends to that x."""
    z, c1, c2, c3, c4 = o.SVDW_G2
    out = []
    for x, y, kind in twist_points_y2_in_fp():
        d = o.f2_sub(c2, x)
        a = o.f2_mul(d, c1)                                            # a u^2 - c3 u + d = 0
        s = o.f2_sqrt(o.f2_sub(o.f2_sqr(c3), o.f2_scal(o.f2_mul(a, d), 4)))
        if s is None:
            continue
        inv2a = o.f2_inv(o.f2_scal(a, 2))
        for u in (o.f2_mul(o.f2_add(c3, s), inv2a), o.f2_mul(o.f2_sub(c3, s), inv2a)):
            if o.map_to_curve_svdw(o._Fp2Ops, o.SVDW_G2, u)[0] == x:
                out.append((u, kind))
    assert sum(k == "real" for _, k in out) >= 2 and sum(k == "imag" for _, k in out) >= 2, out
    return out


@functools.lru_cache(maxsize=None)
def map_cases(g2):
    """rows of two field elements (gnark memory layout) with the oracle's point: the fixture's rows, equal elements (the final addition is
    a doubling), opposite elements (infinity for most), zero on either side, p - 1, the exceptional u, for G2 elements that drive the map onto
    an x1 with g(x1) in Fp, and seeded random rows."""
    rnd = random.Random("wire_cases/map/%d" % g2)
    F, consts = (o._Fp2Ops, o.SVDW_G2) if g2 else (o._FpOps, o.SVDW_G1)
    rand = (lambda: (rnd.randrange(P), rnd.randrange(P))) if g2 else (lambda: rnd.randrange(P))
    enc = o.f2_to_bytes if g2 else o.fp_to_mont_bytes
    fn, to_bytes = (o.map_fields_to_g2, o.g2_to_bytes) if g2 else (o.map_fields_to_g1, o.g1_to_bytes)
    gold = load_golden("hash_to_curve.json")["g2_fields" if g2 else "g1_fields"]
    raw = [("fixture", *(((int(c["u"][0][0]), int(c["u"][0][1])), (int(c["u"][1][0]), int(c["u"][1][1]))) if g2 else (int(c["u"][0]), int(c["u"][1]))))
           for c in gold]
    exc = _exceptional_us(F, consts)
    assert exc and all(F.mul(F.sub(F.one, F.mul(F.mul(u, u), consts[1])), F.add(F.one, F.mul(F.mul(u, u), consts[1]))) == F.zero for u in exc)
    top = [(P - 1, 0), (P - 1, P - 1), (0, P - 1)] if g2 else [P - 1]
    for u in [rand() for _ in range(3)] + [F.small(7)] + exc + top:
        raw += [("equal", u, u), ("opposite", u, F.neg(u)), ("zero_left", F.zero, u), ("zero_right", u, F.zero)]
    raw += [("exceptional", u, v) for u in exc for v in exc]
    raw += [("top", u, v) for u in top for v in top]
    raw.append(("zero_both", F.zero, F.zero))
    if g2:
        us = g2_us_onto_y2_in_fp()
        for i, (u, kind) in enumerate(us):
            raw += [("y2_in_fp_" + kind, u, rand()), ("y2_in_fp_" + kind, rand(), u), ("y2_in_fp_" + kind, u, us[(i + 1) % len(us)][0])]
    raw += [("random", rand(), rand()) for _ in range(32)]
    expect, cases = {}, []
    for cls, u0, u1 in raw:
        if (u0, u1) not in expect:
            expect[(u0, u1)] = to_bytes(fn(u0, u1))
        cases.append(Case(enc(u0) + enc(u1), cls, 1, expect[(u0, u1)]))
    corpus = Corpus(cases)
    n = corpus.counts()
    assert n["fixture"] == len(gold) and n["random"] == 32 and n["equal"] >= 6 and n["exceptional"] >= 1
    # (-u goes to the opposite point unless g(x1) and g(x2) are both squares: x1 and x2 change places under u -> -u)
    assert sum(not any(c.row) for c in cases if c.cls == "opposite") >= 2
    if g2:
        assert n["y2_in_fp_real"] + n["y2_in_fp_imag"] >= 8 and n["y2_in_fp_real"] >= 2 and n["y2_in_fp_imag"] >= 2
    return corpus


# ------------------------------------------------------------------------------------------------ square roots, branch by branch
@functools.lru_cache(maxsize=None)
def sqrt_cases():
    """(fp_squares, fp_non_squares, f2_real [(a0, kind)], f2_squares, f2_non_squares) as integers: the right-hand sides the decode corpus
    takes roots of.  f2_real are the elements of Fp whose root in Fp2 is real (kind "real") or purely imaginary ("imag")."""
    rnd = random.Random("wire_cases/sqrt")
    g1, g2 = GROUPS["g1"], GROUPS["g2"]
    fp_sq = [pt[1] * pt[1] % P for pt in _points("g1")["subgroup"] + _points("g1")["lex_boundary"]] + [0, 1, 4]
    fp_non = [(x ** 3 + o.B_G1) % P for x in (g1.x_without_root(rnd)[0] for _ in range(8))]
    f2_real = [(_g2_rhs(x)[0], kind) for x, _, kind in twist_points_y2_in_fp()] + [(0, "real"), (1, "real"), (P - 1, "imag"), (4, "real"), (P - 4, "imag")]
    f2_sq = [o.f2_sqr(pt[1]) for pt in _points("g2")["subgroup"] + _points("g2")["off_subgroup"]]
    f2_non = [_g2_rhs((w[1], w[0])) for w in (g2.x_without_root(rnd) for _ in range(8))]
    assert all(o.fp_sqrt(a) is None for a in fp_non) and all(o.f2_sqrt(a) is None for a in f2_non)
    assert sum(k == "real" for _, k in f2_real) >= 2 and sum(k == "imag" for _, k in f2_real) >= 2
    return fp_sq, fp_non, f2_real, f2_sq, f2_non
