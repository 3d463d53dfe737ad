"""Adversarial raw-limb cases and a big-integer reference for the data-dependent routines of csrc/fe29.hip.hpp and their one-limb-per-lane
forms (csrc/wide_lds29.hip.hpp, csrc/wide29.hip.hpp).  Plain Python integers and numpy.float32 only: no project code.  Not collected (no
test_ prefix); tests/test_field_primitives.py runs the cases through the compiled header on the CPU, tests/test_limb_ops_gpu.py through
tools/check_limb_ops.hip on the device.

An element is nine signed 29-bit limbs, value = sum v[i] 2^(29 i); the routines choose a multiple k p from a float32 quotient of the top
limb and shift signed limbs arithmetically, so the cases are k p + delta over each routine's whole documented range of k, in every signed
representation its input class admits."""
import random

import numpy as np

U = 4965661367192848881
P = 36 * U**4 + 36 * U**3 + 24 * U**2 + 6 * U + 1
NL, LB = 9, 29
B = 1 << LB
LMASK = B - 1
P_LIMBS = [(P >> (LB * i)) & LMASK for i in range(NL - 1)] + [P >> (LB * (NL - 1))]
P8 = P_LIMBS[NL - 1]
TOP = 1 << (LB * (NL - 1))                                   # 2^232, the weight of the top limb
RP = 1 << (LB * NL)                                          # the Montgomery radix 2^261
RP_INV = pow(RP, -1, P)
I32 = 1 << 31
MODES = ("min", "max", "rand", "nonneg")

# operation numbers shared by tools/bounds_check.cpp (hc_fe_primitive) and tools/check_limb_ops.hip
OP_NORM, OP_MUL8_NORM, OP_HALVE, OP_REDUCE, OP_REDUCE_ARITH, OP_REDUCE_ARITH_NORM, OP_CYCLO_OUT, OP_CANONICAL, OP_IS_ZERO = range(9)
OP_NAMES = ["fe_norm", "fe_mul8_norm", "fe_halve", "fe_reduce", "fe_reduce_arith", "fe_reduce_arith_norm", "fe_cyclo_out", "fe_canonical", "fe_is_zero"]
# one-limb-per-lane operations of WideLds::LimbOps (kernel (b) of the device program); the last two are the compounds of wide_double_step
L_NORM, L_HALVE, L_ADD, L_SUB, L_DBL, L_NEG, L_SEL, L_NORM_SUB, L_HALVE_CHAIN = range(9)


def value(limbs):
    """the represented integer"""
    return sum(int(v) << (LB * i) for i, v in enumerate(limbs))


def representations(V, slack, mode, rng=None, floor=None):
    """Nine signed limbs for V: limbs 0..7 in turn take r = rest mod 2^29, r -+ 2^29 or r - 2^30, each only where it stays within
    [floor, 2^29 + slack] (floor: -2^29 - slack unless given); mode picks the smallest candidate, the largest, a random one, or a random
    non-negative one.  The top limb takes what is left and must fit int32."""
    lo = -B - slack if floor is None else floor
    rest, limbs = V, []
    for _ in range(NL - 1):
        r = rest % B
        cands = [c for c in (r - 2 * B, r - B, r, r + B) if lo <= c <= B + slack and (mode != "nonneg" or c >= 0)]
        c = cands[0] if mode == "min" else cands[-1] if mode == "max" else rng.choice(cands)
        limbs.append(c)
        rest = (rest - c) >> LB
    assert -I32 <= rest < I32, "top limb outside int32"
    return limbs + [rest]


def nearest_k(V):
    """round(V / p), halves up: the multiple of p a value reduction has to take off (from the big integer alone)"""
    return (2 * V + P) // (2 * P)


def reach(values):
    return {nearest_k(V) for V in values}


def assert_reach(values, k_lo, k_hi):
    """a condition on the INPUTS: the cases reach every k in [-8, 8] (as far as the range goes) and both ends of the documented range"""
    ks = reach(values)
    missing = [k for k in range(max(-8, k_lo), min(8, k_hi) + 1) if k not in ks] + [k for k in (k_lo, k_hi) if k not in ks]
    assert not missing and min(ks) >= k_lo and max(ks) <= k_hi, (missing, min(ks), max(ks))
    return ks


# ------------------------------------------------------------------------------------------------ limb-exact restatements
def _i32(v):
    assert -I32 <= v < I32, "int32 overflow in the restatement: the case is outside the routine's input class"
    return v


def float_k(top):
    """(int32_t)rintf((float)top * (1.0f / (float)P8))"""
    return int(np.rint(np.float32(top) * (np.float32(1.0) / np.float32(P8))))


def fe_norm(a):
    return [a[0] & LMASK] + [_i32((a[i] & LMASK) + (a[i - 1] >> LB)) for i in range(1, NL - 1)] + [_i32(a[NL - 1] + (a[NL - 2] >> LB))]


def fe_mul8_norm(a):
    m26 = (1 << (LB - 3)) - 1
    return [(a[0] & m26) << 3] + [_i32(((a[i] & m26) << 3) + (a[i - 1] >> (LB - 3))) for i in range(1, NL - 1)] + [_i32(a[NL - 1] * 8 + (a[NL - 2] >> (LB - 3)))]


def fe_halve(a):
    t = [_i32(a[i] + (P_LIMBS[i] if a[0] & 1 else 0)) for i in range(NL)]
    return [_i32((t[i] >> 1) + ((t[i + 1] & 1) << (LB - 1))) for i in range(NL - 1)] + [t[NL - 1] >> 1]


def fe_reduce_arith(a):
    k = float_k(a[NL - 1])
    out, hi_prev = [], 0
    for i in range(NL):
        t = k * P_LIMBS[i]
        out.append(_i32(a[i] - ((t & LMASK) if i < NL - 1 else t) - hi_prev))
        hi_prev = t >> LB
    return out


def kp_row(k):
    """row k of F29_KP: limbs 0..7 of k p in [0, 2^29), the top limb signed"""
    v = k * P
    return [(v >> (LB * i)) & LMASK for i in range(NL - 1)] + [v >> (LB * (NL - 1))]


def fe_reduce(a):
    row = kp_row(max(-256, min(256, float_k(a[NL - 1]))))
    return [_i32(a[i] - row[i]) for i in range(NL)]


def fe_reduce_arith_norm(a):
    return fe_norm(fe_reduce_arith(a))


def fe_cyclo_out(t, x):
    w = [_i32(3 * t[i] - 2 * x[i]) for i in range(NL)]
    row = kp_row(max(-256, min(256, float_k(w[NL - 1]))))
    return fe_norm([_i32(w[i] - row[i]) for i in range(NL)])


def fe_canonical(a):
    v = value(a) % P
    return [(v >> (LB * i)) & LMASK for i in range(NL - 1)] + [v >> (LB * (NL - 1))]


def fe_add(a, b): return [_i32(x + y) for x, y in zip(a, b)]
def fe_sub(a, b): return [_i32(x - y) for x, y in zip(a, b)]
def fe_neg(a): return [-x for x in a]


def xi_half(mine, other, h):
    """wide_xi_half: one component of (9 + i)(mine + other i) seen from `mine`, not normalised"""
    return fe_add(fe_add(fe_mul8_norm(mine), mine), other if h else fe_neg(other))


RESTATED = {OP_NORM: fe_norm, OP_MUL8_NORM: fe_mul8_norm, OP_HALVE: fe_halve, OP_REDUCE: fe_reduce, OP_REDUCE_ARITH: fe_reduce_arith,
            OP_REDUCE_ARITH_NORM: fe_reduce_arith_norm, OP_CANONICAL: fe_canonical}


def limb_op(op, a, b, c):
    """what component c of a WideLds::limbs phase of kernel (b) must leave, from the Fe-level restatements"""
    if op == L_NORM: return fe_norm(a)
    if op == L_HALVE: return fe_halve(a)
    if op == L_ADD: return fe_add(a, b)
    if op == L_SUB: return fe_sub(a, b)
    if op == L_DBL: return fe_add(a, a)
    if op == L_NEG: return fe_neg(a)
    if op == L_SEL: return a if c & 1 else b
    if op == L_NORM_SUB: return fe_norm(fe_sub(a, fe_add(fe_add(b, b), b)))               # y' = G^2 - 3 E^2
    if op == L_HALVE_CHAIN: return fe_norm(fe_halve(fe_norm(fe_add(a, b))))               # G = (B + F) / 2
    raise ValueError(op)


# ------------------------------------------------------------------------------------------------ case sets
def tie_values(k, rng):
    """values whose top limb sits within three units of (k + 1/2) P8, carries of the representation included: the float quotient of
    the top limb is k + 1/2 up to its last place, and rintf takes either neighbour"""
    return [(((2 * k + 1) * P8) // 2 + n) * TOP + rng.randrange(TOP) for n in (-3, -2, -1, 0, 1, 2, 3)]


def deltas(rng, n_random=2):
    half = P // 2
    return [0, 1, -1, half, half + 1, -half] + [rng.randrange(-half, half + 1) for _ in range(n_random)]


def reduction_cases(seed=1, k_max=255, slack=1024, floor=None):
    """(V, limbs): k p + delta in a signed representation of slack `slack`, |V| < (k_max + 1) p.  Every k of the range meets delta = 0 and
    the rounding ties; the k near zero, the ends and a few in between meet every delta.  Modes go round."""
    rng = random.Random(seed)
    dense = set(range(-8, 9)) | {k_max, -k_max, k_max - 1, 1 - k_max, 128, -128, 127, -127, 64, -64} | {rng.randrange(-k_max, k_max + 1) for _ in range(12)}
    out, n = [], 0
    for k in range(-k_max, k_max + 1):
        ties = tie_values(k, rng)
        for V in [k * P + d for d in (deltas(rng) if k in dense else [0])] + (ties if k in dense else ties[2:5]):
            if not -k_max <= nearest_k(V) <= k_max:                     # stay within k_max p + p / 2
                continue
            mode = MODES[n % 4]
            n += 1
            out.append((V, representations(V, slack, mode, rng, floor)))
    # rows written limb by limb: every limb at an end of the class (a random value comes within `slack` of an end once in 2^19 limbs)
    e_lo, e_hi = -B - slack if floor is None else floor, B + slack
    for k in (-k_max + 1, -128, -3, 0, 1, 2, 127, k_max - 1):
        for low in ([e_lo] * 8, [e_hi] * 8, [e_lo, e_hi] * 4, [e_hi, e_lo] * 4, [e_lo, 0, e_hi, -1] * 2):
            row = low + [k * P8 + rng.randrange(-P8 // 4, P8 // 4)]
            out.append((value(row), row))
    return out


def is_zero_cases(seed=2):
    """(V, limbs, expected): every representation mode of k p for |k| <= 127 (true), and k p + delta for the deltas the filter must
    not let through or must send to the exact path (false).  Slack 64, the class fe_is_zero documents."""
    rng = random.Random(seed)
    out = []
    for k in range(-127, 128):
        for mode in MODES:
            out.append((k * P, representations(k * P, 64, mode, rng), True))
    n = 0
    for k in list(range(-127, 128, 3)) + [127, -127, 126, -126, 101, -101, 0, 1, -1]:
        for d in (1, -1, TOP, -TOP, 130 * TOP, -130 * TOP, 136 * TOP, -136 * TOP, rng.randrange(1, P // 2), -rng.randrange(1, P // 2)):
            V = k * P + d
            out.append((V, representations(V, 64, MODES[n % 4], rng), False))
            n += 1
    return out


def zero_filter_remainder(limbs):
    """what fe_is_zero's filter compares with its window: the top limb's distance from the nearest multiple of P8 (exact integers)"""
    top = limbs[NL - 1]
    return top - ((2 * top + P8) // (2 * P8)) * P8


# the largest remainder a true zero k p, |k| <= 127, of the class can show: floor(127 (p mod 2^232) / 2^232) = 56 from the value and up to
# two units of carry from limbs below -2^29 (one where every limb is negative; the second needs a limb below -2^29, 64 values in 2^29)
ZERO_REMAINDER_REACHED = 127 * (P % TOP) // TOP + 1


def canonical_cases(seed=3):
    """(V, limbs): values over (-4p, 4p), the ends +-(4p - 1) in every mode"""
    rng = random.Random(seed)
    vals = [s * (4 * P - 1) for s in (1, -1) for _ in MODES] + [s * (4 * P - 2) for s in (1, -1)]
    for q in range(-4, 4):
        vals += [q * P + d for d in (0, 1, P - 1, P // 2, P // 2 + 1, rng.randrange(P), rng.randrange(P))]
    vals = [V for V in vals if abs(V) < 4 * P]
    return [(V, representations(V, 1024, MODES[i % 4], rng)) for i, V in enumerate(vals)]


def cyclo_out_cases(seed=4):
    """(W, t, x): W = 3 t - 2 x = k p + delta over k in [-255, 255] with 3 |t| + 2 |x| < 256 p (what the harness admits); t and x in the
    class the header names for them, limbs 0..7 within [-2^4, 2^29 + 2^4]"""
    rng = random.Random(seed)
    out = []
    for n, (W, _) in enumerate(reduction_cases(seed, 255, 0)):
        room = 256 * P - abs(W) - 8                                  # 2 |x| + the rounding of t must fit here
        xmax = min(40 * P, room // 5)
        x = rng.randrange(-xmax, xmax + 1) if xmax > 0 else 0
        while (W + 2 * x) % 3:                                       # make W + 2 x a multiple of 3
            x += 1
        t = (W + 2 * x) // 3
        if 3 * abs(t) + 2 * abs(x) >= 256 * P - 4:
            continue
        mt, mx = MODES[n % 4], MODES[(n // 4) % 4]
        out.append((W, representations(t, 16, mt, rng, floor=-16), representations(x, 16, mx, rng, floor=-16)))
    return out


EDGE_LIMBS = (0, -1, 1, LMASK, B, -B, B + 1, -B - 1, LMASK - 1, 3 * B - 1, -3 * B, 2 * B, -2 * B + 1, 2 * B - 1)


def raw_cases(seed, top_bound, limb_bound, n_random=400):
    """rows of raw limbs for fe_norm / fe_mul8_norm / fe_halve: all limbs -1, a negative limb directly above a zero limb, every edge limb
    next to every other, and random limbs up to the bound"""
    rng = random.Random(seed)
    edges = [e for e in EDGE_LIMBS if -limb_bound <= e <= limb_bound] + [limb_bound, -limb_bound]
    tops = [t for t in (0, 1, -1, P8, -P8, P8 + 2, top_bound, -top_bound, 255 * P8 + 1, -255 * P8) if abs(t) <= top_bound]
    rows = [[-1] * NL, [0] * NL, [LMASK] * (NL - 1) + [P8], [-B] * (NL - 1) + [-1], [0, -1] * 4 + [1], [-B - 1, 0] * 4 + [-2]]
    for a in edges:
        for b in edges:
            rows.append([a, b, 0, a, a, b, b, a, rng.choice(tops)])
    for _ in range(n_random):
        rows.append([rng.choice(edges) if rng.random() < 0.3 else rng.randrange(-limb_bound, limb_bound + 1) for _ in range(NL - 1)] + [rng.choice(tops) if rng.random() < 0.5 else rng.randrange(-top_bound, top_bound + 1)])
    return rows


NORM_LIMB_BOUND = 3 * B - 1          # fe_norm: any limb whose carry leaves the limb above inside int32
HALVE_LIMB_BOUND = 3 * B - 1         # fe_halve: a limb plus a limb of p stays inside int32


def n_class_operands(seed, n_random):
    """N-class rows (limbs 0..7 in [0, 2^29), the top limb signed and small: what a product leaves) for the product tests: all-ones
    limbs, zero, p - 1, +-k p with the top limb at the edge of the class, and random values of (-eps p, (1 + eps) p)"""
    rng = random.Random(seed)

    def n_class(V):
        return [(V >> (LB * i)) & LMASK for i in range(NL - 1)] + [V >> (LB * (NL - 1))]
    rows = [[LMASK] * (NL - 1) + [P8 + 2], [LMASK] * (NL - 1) + [-2], [0] * NL, n_class(P - 1), n_class(P), n_class(-P // 1024), n_class(1), n_class(-1),
            [LMASK] * (NL - 1) + [0], [0] * (NL - 1) + [P8 + 2], [0] * (NL - 1) + [-2]]
    rows += [n_class(rng.randrange(-P // 1024, P + P // 1024)) for _ in range(n_random)]
    return rows


# ------------------------------------------------------------------------------------------------ one limb per lane: whole phases
MAX_COMP = 7
# (limb bound, top-limb bound) of the operand rows of each operation of kernel (b): what keeps every intermediate inside int32
LIMB_OP_BOUNDS = {L_NORM: (NORM_LIMB_BOUND, 1 << 30), L_HALVE: (HALVE_LIMB_BOUND, 1 << 30), L_ADD: (2 * B - 1, 1 << 29), L_SUB: (2 * B - 1, 1 << 29),
                  L_DBL: (2 * B - 1, 1 << 29), L_NEG: (2 * B - 1, 1 << 29), L_SEL: (2 * B - 1, 1 << 29), L_NORM_SUB: (B - 1, 1 << 28), L_HALVE_CHAIN: (2 * B - 1, 1 << 29)}


def boundary_rows(e, t):
    """rows that show a carry or a parity crossing from one component into the next (limb bound e, top bound t): a large negative top
    limb (its carry must not reach limb 0 of the component above), zero (must receive nothing), all limbs -1, negative limbs directly
    above zero limbs, an odd value with an odd top limb, an even limb 0 under odd limbs"""
    return [[LMASK] * 8 + [1 - t], [0] * NL, [-1] * NL, [0, -e] * 4 + [t - 1], [1, 0, 0, 0, 0, 0, 0, 0, 2 * (t // 4) + 1], [2, 1, 1, 1, 1, 1, 1, 1, 3],
            [e] * 8 + [-3], [-e, 0, e, -1, 1 - e, e - 1, -2, e] + [t - 2], [e - 1, -e] * 4 + [-(t // 2) - 1]]


def limb_phase_cases(seed=20):
    """(op, n_comp, a rows, b rows) for WideLds::limbs: every operation at 1..7 components, the boundary rows in three rotations and
    random rows"""
    rng = random.Random(seed)
    out = []
    for op, (e, t) in LIMB_OP_BOUNDS.items():
        special, pool = boundary_rows(e, t), raw_cases(seed + op, t, e, 60)
        for n_comp in range(1, MAX_COMP + 1):
            for variant in range(4):
                if variant < 3:
                    a = [special[(3 * variant + c) % len(special)] for c in range(n_comp)]
                    b = [special[(3 * variant + 2 * c + 1) % len(special)] for c in range(n_comp)]
                else:
                    a, b = [rng.choice(pool) for _ in range(n_comp)], [rng.choice(pool) for _ in range(n_comp)]
                out.append((op, n_comp, a, b))
    return out


# ------------------------------------------------------------------------------------------------ the cyclotomic output step on slots
CYCLO_AB = {0: (4, 0), 1: (2, 3), 2: (5, 1), 3: (5, 1), 4: (4, 0), 5: (2, 3)}      # output slot k -> squares (A, B); k >= 3 also S: 8, 6, 7
CYCLO_S = {3: 8, 4: 6, 5: 7}


def cyclo_out_expected(prod, a):
    """wide_cyclo_out_limbs from the Fe-level restatements.  prod[l][h], a[k][h]: rows.  -> (limbs[k][h], W[k][h]) with W the big integer
    3 t -+ 2 x the step reduces (from value() alone, no restatement)"""
    limbs, W = [[None, None] for _ in range(6)], [[None, None] for _ in range(6)]
    for k in range(6):
        A, Bq = CYCLO_AB[k]
        for h in (0, 1):
            x = a[k][h]
            if k < 3:
                X = fe_norm(xi_half(prod[A][h], prod[A][1 - h], h))
                t = fe_norm(fe_add(X, prod[Bq][h]))
                dd = fe_norm(fe_sub(t, x))
                U = [value(prod[A][0]), value(prod[A][1])]
                tv = (9 * U[h] + (U[0] if h else -U[1])) + value(prod[Bq][h])
                W[k][h] = 3 * tv - 2 * value(x)
            else:
                S = CYCLO_S[k]
                d = [fe_norm(fe_sub(fe_sub(prod[S][j], prod[A][j]), prod[Bq][j])) for j in (0, 1)]
                t = fe_norm(xi_half(d[h], d[1 - h], h)) if k == 3 else d[h]
                dd = fe_norm(fe_add(t, x))
                dv = [value(prod[S][j]) - value(prod[A][j]) - value(prod[Bq][j]) for j in (0, 1)]
                tv = (9 * dv[h] + (dv[0] if h else -dv[1])) if k == 3 else dv[h]
                W[k][h] = 3 * tv + 2 * value(x)
            limbs[k][h] = fe_reduce_arith(fe_norm(fe_add(fe_add(dd, dd), t)))
    return limbs, W


def cyclo_out_slot_cases(seed=30, n=256):
    """(alias, prod[9][2], a[6][2]): the nine product slots hold N-class extremes and random N-class rows (what the squarings leave), `a`
    N-class rows or reduced values in the class of a reduction's output.  Whole slots of extremes drive the multiplier far from zero:
    S small under A, B large gives 3 xi (S - A - B) near -57 p."""
    rng = random.Random(seed)
    rows = n_class_operands(seed, 40)
    lows = [r for r in rows if value(r) * 8 < P] or rows
    highs = [r for r in rows if value(r) * 8 > 7 * P]
    out = []
    for i in range(n):
        style = i % 4
        prod = []
        for l in range(9):
            if style == 0: pick = lambda: rng.choice(rows)
            elif style == 1: pick = lambda: rng.choice(lows if l >= 6 else highs)             # sums small, squares large: k far below zero
            elif style == 2: pick = lambda: rng.choice(highs if l >= 6 else lows)
            else: pick = lambda: rng.choice(highs if rng.random() < 0.5 else lows)
            prod.append([pick(), pick()])
        a = []
        for k in range(6):
            half = []
            for h in (0, 1):
                if rng.random() < 0.5:
                    half.append(rng.choice(rows))
                else:
                    V = rng.choice([rng.randrange(-P * 51 // 100, P * 51 // 100), P // 2, -(P // 2), 0, -1])
                    half.append(representations(V, 16, rng.choice(MODES), rng, floor=-16))
            a.append(half)
        out.append((i & 1, prod, a))
    return out


# ------------------------------------------------------------------------------------------------ the wide Fp12 operations
W_MUL, W_SQR, W_MUL_LINE, W_CYCLO_SQR = range(4)


def wide_cases(seed=40, n_each=16, n_helper=64):
    """(op, A[6][2], B[6][2]) on N-class operands; -> (records for one wavefront, wide_mul records for the run with the helper wave)"""
    rng = random.Random(seed)
    rows = n_class_operands(seed, 64)
    extremes = rows[:11]

    def val(i):
        return [[rng.choice(extremes if i % 4 == 0 else rows) for _ in (0, 1)] for _ in range(6)]
    one = [(op, val(i), val(i + 1)) for op in (W_MUL, W_SQR, W_MUL_LINE, W_CYCLO_SQR) for i in range(n_each)]
    two = [(W_MUL, val(i), val(i + 2)) for i in range(n_helper)]
    return one, two


def from_mont(row):
    """the field element a slot half stands for: value / 2^261 mod p"""
    return value(row) * RP_INV % P
