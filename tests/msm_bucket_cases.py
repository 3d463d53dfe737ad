"""Structured inputs that STAY on the bucket path of csrc/gpbc_msm.hip and make its exceptional group-law cases happen where they are named
(not collected: no test_ prefix).  tests/test_bucket_msm_cases.py (CPU) and tests/test_bucket_msm_structured_gpu.py build on it.

Two devices keep the scalars random — so that the skew detector of msm_run stays quiet — and still decide every intermediate value:
  * KNOWN DISCRETE LOGS.  Every base is [a_i]G, so the exact result is [sum a_i k_i mod r]G: one big-integer dot product here and one
    scalar multiplication by the oracle.  No engine kernel has a part in the expected value.
  * CANCELLING FILLER.  Terms (P_j, k_j) and (-P_j, k_j) with k_j uniform in 256 bits add infinity to every bucket they both meet; they
    make a case long enough for the bucket path, and a hand-placed SKELETON of a few terms then decides bucket sums, group values,
    window sums and Horner steps.  -P_j is p - y on the stored residue (negate_rows), not an engine call.
The filler comes in two layouts because of the partial top window at c = 12, whose key is (i mod 256) * 16 + digit: partners at
ADJACENT indices land in different sub-buckets there and cancel only in the tree sum; partners 256 APART share a bucket.

Two checks certify the INPUTS (neither ever supplies an expected output):
  * longest_bucket(): k_msm_keys restated in numpy, sub-bucket bits included; every case stays at or below half of bucket_cap().
  * Model: the plan with points as integers mod r (0 = infinity) — bucket sums, groups of MSM_GROUP digits as k_msm_groups forms them
    (lo = first & dmask, running, total, the lo - 1 multiple), the fan-in-8 tree level by level, Horner — recording at every addition
    whether an operand is infinite or the operands are equal or opposite.  Each case lists the events it is named after (Case.checks)
    and the model must confirm them.  Bucket order on the device follows the atomics, so the bucket stage records as certain only what
    holds for EVERY order of a bucket's members (`bucket:sum_inf`: the last addition meets its opposite; `bucket:all_equal`: the second
    addition meets its own accumulator); what holds in ascending index order is recorded apart (`bucket:idx_*`) and certifies nothing.
    No bucket can promise "through infinity and on" in every order (the order with one sign first avoids it): that event is certified
    where the order is fixed — the running sum of a group, the tree, Horner.
plan="host" models tools/bounds_check.cpp msm_host instead (plain top digits, one chain over a window's groups) for the reduced cases."""
import functools
import os
import re

import numpy as np

import bn254_py as o
from conftest import ROOT

R = o.R
_CSRC = os.path.join(ROOT, "gopairingbasedcryptography_amd", "csrc")


def _constant(header, name):
    text = open(os.path.join(_CSRC, header)).read()
    return int(re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))


MSM_MIN_TERMS = _constant("gpbc_common.hpp", "MSM_MIN_TERMS")
MSM_MAX_BUCKET_BASE = _constant("gpbc_common.hpp", "MSM_MAX_BUCKET_BASE")
MSM_GROUP = _constant("msm29.hip.hpp", "MSM_GROUP")
MSM_FAN = _constant("gpbc_msm.hip", "MSM_FAN")
SUB_STRIDE = 256                                      # 2^12 keys / 2^4 digit values: sub-buckets of the partial top window at c = 12
# the smallest shapes that reach each plan (msm_plan: c = 16 from 2^17 terms on, else 12), and the reduced ones for msm_host
SHAPES = ((12, MSM_MIN_TERMS + 6), (16, (1 << 17) + 6))
REDUCED = ((5, 70), (8, 70))


def window_bits(n):
    """msm_plan of csrc/gpbc_msm.hip: p.c = n >= 2^17 ? 16 : 12"""
    return 16 if n >= 1 << 17 else 12


def bucket_cap(n, c):
    """the longest bucket msm_run accepts, csrc/gpbc_msm.hip msm_run: `if (longest > MSM_MAX_BUCKET_BASE + 8 * (uint32_t)(n >> p.c))`"""
    return MSM_MAX_BUCKET_BASE + 8 * (n >> c)


def n_windows(c):
    return -(-256 // c)


def top_bits(c):
    return 256 - c * (n_windows(c) - 1)


def digits(K, c):
    """msm_digit for every term and window: K uint8 (n, 32) little-endian -> int64 (n, W)"""
    k64 = np.ascontiguousarray(K).view("<u8").reshape(-1, 4)
    W = n_windows(c)
    out = np.zeros((k64.shape[0], W), dtype=np.int64)
    for w in range(W):
        bit = w * c
        wi, sh = bit >> 6, bit & 63
        v = k64[:, wi] >> np.uint64(sh)
        if sh + c > 64 and wi + 1 < 4:
            v = v | (k64[:, wi + 1] << np.uint64(64 - sh))
        out[:, w] = (v & np.uint64((1 << c) - 1)).astype(np.int64)
    return out


def keys(K, inf, c, plan="device"):
    """k_msm_keys: the key of every (term, window) inside its window, 0 = no entry (digit 0 or a base at infinity); in a partial top
    window the device puts the sub-bucket i mod S above the digit"""
    D = digits(K, c)
    D[np.asarray(inf, dtype=bool)] = 0
    tb = top_bits(c)
    if plan == "device" and tb < c:
        sub = (np.arange(D.shape[0], dtype=np.int64) & ((1 << (c - tb)) - 1)) << tb
        D[:, -1] = np.where(D[:, -1] != 0, D[:, -1] | sub, 0)
    return D


def longest_bucket(D, c):
    return max(int(np.bincount(D[:, w], minlength=2)[1:].max()) for w in range(D.shape[1]))


# ------------------------------------------------------------------------------------------------------------------------- cases
POOL_SIZE = (1 << 17) + 16


@functools.lru_cache(maxsize=None)
def pool():
    """the logs of the filler / random bases, shared by every case so that their points are computed once per group"""
    raw = np.random.default_rng(0xB0C4E7).bytes(32 * POOL_SIZE)
    return [int.from_bytes(raw[32 * j:32 * j + 32], "little") % (R - 1) + 1 for j in range(POOL_SIZE)]


def named_log(tag):
    return o.bench_scalar("bucket-case-" + tag, 0) % (R - 1) + 1


class Case:
    """n terms: base i is [logs[i]]G, negated (p - y) where neg[i]; logs[i] == 0 is the point at infinity.  src[i] >= 0 says that
    logs[i] is pool()[src[i]].  scalars: uint8 (n, 32).  expect_log: the discrete log of the exact sum.  checks: [(text, f(model))]."""
    def __init__(self, name, c, plan, logs, neg, src, scalars):
        self.name, self.c, self.plan, self.n = name, c, plan, len(logs)
        self.logs, self.neg, self.src, self.scalars = logs, np.asarray(neg, dtype=bool), np.asarray(src, dtype=np.int64), np.ascontiguousarray(scalars)
        self.checks = []
        eff = self.effective_logs()
        raw = self.scalars.tobytes()
        self.expect_log = sum(a * int.from_bytes(raw[32 * i:32 * i + 32], "little") for i, a in enumerate(eff) if a) % R

    def effective_logs(self):
        return [(R - a) % R if s else a for a, s in zip(self.logs, self.neg)]

    def keys(self):
        return keys(self.scalars, np.array([a == 0 for a in self.logs]), self.c, self.plan)

    def expect(self, text, fn):
        self.checks.append((text, fn))


def digit_scalar(c, placement):
    """the scalar whose digit in window w is placement[w] and 0 elsewhere"""
    k = 0
    for w, d in placement.items():
        assert 0 < d < 1 << (top_bits(c) if w == n_windows(c) - 1 else c), (c, w, d)
        k += d << (c * w)
    assert k < 1 << 256
    return k


def assemble(name, c, n, plan, placed, layout, seed, infinities=0):
    """placed: {index: (log, scalar or None for a random one)}; `infinities` more bases at infinity with random scalars spread through
    the call; every other index gets cancelling filler in the given layout ("adjacent" or "apart": partner SUB_STRIDE further on)."""
    rng = np.random.default_rng(seed)
    K = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    placed = dict(placed)
    for j in range(infinities):
        i = (j + 1) * n // (infinities + 1) + 1
        while i in placed:
            i += 1
        placed[i] = (0, None)
    if (n - len(placed)) % 2:
        i = n - 1
        while i in placed:
            i -= 1
        placed[i] = (0, None)                                      # one more infinity keeps the filler in pairs
    logs, neg, src = [None] * n, np.zeros(n, dtype=bool), np.full(n, -1, dtype=np.int64)
    for i, (a, k) in placed.items():
        logs[i] = a % R
        if k is not None:
            K[i] = np.frombuffer(k.to_bytes(32, "little"), dtype=np.uint8)
    free = [i for i in range(n) if logs[i] is None]
    if layout == "adjacent":
        pairs = list(zip(free[0::2], free[1::2]))
    else:
        assert layout == "apart"
        pairs, left, open_ = [], [], set(free)
        for i in free:
            if i not in open_:
                continue
            open_.discard(i)
            if i + SUB_STRIDE in open_:
                open_.discard(i + SUB_STRIDE)
                pairs.append((i, i + SUB_STRIDE))
            else:
                left.append(i)
        pairs += list(zip(left[0::2], left[1::2]))
    P = pool()
    for j, (i0, i1) in enumerate(pairs):
        logs[i0] = logs[i1] = P[j]
        src[i0] = src[i1] = j
        neg[i1] = True
        K[i1] = K[i0]
    return Case(name, c, plan, logs, neg, src, K)


def _random_scalar_all_digits_live(c, seed):
    rng = np.random.default_rng(seed)
    while True:
        k = int.from_bytes(rng.bytes(32), "little")
        if all((k >> (c * w)) & ((1 << c) - 1) for w in range(n_windows(c))):
            return k


def _has(m, name, *row):
    rows = m.events.get(name)
    return rows is not None and bool((rows[:, :len(row)] == np.array(row, dtype=np.int64)).all(axis=1).any())


def _count(m, name, w=None):
    rows = m.events.get(name)
    return 0 if rows is None else len(rows) if w is None else int((rows[:, 0] == w).sum())


def _windows(c, plan):
    """every window on the device plan (the shapes there are large enough for each window to show an event); any one on the host"""
    return range(n_windows(c)) if plan == "device" else (None,)


def case_one_base(c, n, plan):
    a = named_log("one-base")
    rng = np.random.default_rng(101)
    K = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    logs = [a] * n
    for i in (3, n // 3, n // 2, n - 2):
        logs[i] = 0                                                # bases at infinity
    case = Case("one_base", c, plan, logs, np.zeros(n, dtype=bool), np.full(n, -1), K)
    for w in _windows(c, plan):
        case.expect("window %s: a bucket of equal points only — its second addition meets its own accumulator in every order" % w,
                    lambda m, w=w: _count(m, "bucket:all_equal", w) >= 1)
    case.expect("no bucket sum is infinite", lambda m: _count(m, "bucket:sum_inf") == 0)
    return case


def case_p_and_minus_p(c, n, plan):
    a = named_log("p-and-minus-p")
    rng = np.random.default_rng(102)
    K = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    case = Case("p_and_minus_p", c, plan, [a] * n, rng.integers(0, 2, size=n).astype(bool), np.full(n, -1), K)
    for w in _windows(c, plan):
        case.expect("window %s: a bucket whose sum is infinity (its last addition meets the opposite point in every order)" % w,
                    lambda m, w=w: _count(m, "bucket:sum_inf", w) >= 1)
        case.expect("window %s: a running sum that passes through infinity and carries on" % w,
                    lambda m, w=w: _count(m, "group.running:opposite", w) >= 1 and _count(m, "group.running:reborn", w) >= 1)
    case.expect("a bucket of equal points only", lambda m: _count(m, "bucket:all_equal") >= 1)
    case.expect("a tree chain that passes through infinity and carries on", lambda m: plan == "host" or _count(m, "tree:reborn") >= 1)
    return case


def case_pairs_only(c, n, plan, layout):
    case = assemble("pairs_only_" + layout, c, n, plan, {}, layout, 103)
    W = n_windows(c)
    case.expect("the sum is infinity", lambda m: case.expect_log == 0 and m.result == 0 and _count(m, "result:inf") == 1)
    case.expect("every window sum is infinity", lambda m: all(s == 0 for s in m.window_sums))
    case.expect("every bucket of a full window is infinite by its last addition",
                lambda m: all(_count(m, "bucket:sum_inf", w) == m.used_buckets[w] > 0 for w in range(W - (top_bits(c) < c))))
    if plan == "device" and top_bits(c) < c:
        if layout == "adjacent":
            case.expect("partial top window: partners in different sub-buckets, live buckets, cancelling in the tree only",
                        lambda m: _count(m, "bucket:sum_inf", W - 1) == 0 and m.live_buckets[W - 1] > 0 and _count(m, "tree:opposite", W - 1) >= 1)
        else:
            # (the n mod 512 terms left over at the end pair up as neighbours: at most that many live buckets)
            case.expect("partial top window: partners share a sub-bucket", lambda m: m.live_buckets[W - 1] <= n % (2 * SUB_STRIDE) and
                        _count(m, "bucket:sum_inf", W - 1) >= m.used_buckets[W - 1] - n % (2 * SUB_STRIDE) > 0)
    return case


def case_pairs_plus_lone(c, n, plan):
    a, k = named_log("lone"), _random_scalar_all_digits_live(c, 104)
    case = assemble("pairs_plus_lone", c, n, plan, {0: (a, k)}, "adjacent", 104, infinities=3)
    ds = [(k >> (c * w)) & ((1 << c) - 1) for w in range(n_windows(c))]
    case.expect("every window sum is the lone term's digit multiple", lambda m: all(s == d * a % R for s, d in zip(m.window_sums, ds)))
    case.expect("one live bucket per full window", lambda m: all(m.live_buckets[w] == 1 for w in range(n_windows(c) - (top_bits(c) < c))))
    case.expect("bases at infinity among the terms", lambda m: sum(1 for x in case.logs if x == 0) >= 3)
    return case


def case_sum_zero_closing(c, n, plan):
    P = pool()
    rng = np.random.default_rng(105)
    K = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw = K.tobytes()
    ac = named_log("closing")
    partial = sum(P[i] * int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(n - 1)) % R
    K[n - 1] = np.frombuffer(((R - partial) * pow(ac, -1, R) % R).to_bytes(32, "little"), dtype=np.uint8)
    src = np.arange(n); src[n - 1] = -1
    case = Case("sum_zero_closing", c, plan, P[:n - 1] + [ac], np.zeros(n, dtype=bool), src, K)
    quiet = ["bucket:sum_inf", "group.running:opposite", "group.running:reborn", "group.total:opposite", "group.total:reborn", "group.multiple:opposite",
             "group.mul_small:inf_running", "tree:opposite", "tree:reborn", "horner:reborn", "horner:dbl_inf"]
    case.expect("the sum is infinity", lambda m: case.expect_log == 0 and m.result == 0)
    case.expect("infinity appears at the last Horner addition and nowhere before",
                lambda m: [tuple(r) for r in m.events.get("horner:opposite", ())] == [(0,)] and all(_count(m, q) == 0 for q in quiet))
    return case


def case_group_total_cancels(c, n, plan):
    """B_hi = P, B_{hi-1} = -2P in group 2 of window 3: at digit hi - 1  running = -P = -total"""
    a, w, g = named_log("group-total"), 3, 2
    hi = g * MSM_GROUP + MSM_GROUP - 1
    placed = {0: (a, digit_scalar(c, {w: hi})), 1: (R - 2 * a % R, digit_scalar(c, {w: hi - 1}))}
    case = assemble("group_total_cancels", c, n, plan, placed, "apart", 106, infinities=2)
    case.expect("total = -running at digit hi - 1", lambda m: _has(m, "group.total:opposite", w, g, MSM_GROUP - 2))
    case.expect("total leaves infinity again at the next digit, then meets an equal running sum",
                lambda m: _has(m, "group.total:reborn", w, g, MSM_GROUP - 3) and _has(m, "group.total:equal", w, g, MSM_GROUP - 4))
    return case


def case_group_running_cancels(c, n, plan):
    """B_hi = P, B_lo = -P in the TOP group of window 5: running ends infinite, total = 7P does not, and the multiplier is 2^c - 9"""
    a, w, g = named_log("group-running"), 5, (1 << c) // MSM_GROUP - 1
    placed = {0: (a, digit_scalar(c, {w: (1 << c) - 1})), 1: (R - a, digit_scalar(c, {w: (1 << c) - MSM_GROUP}))}
    case = assemble("group_running_cancels", c, n, plan, placed, "adjacent", 107)
    case.expect("running meets its opposite at digit lo", lambda m: _has(m, "group.running:opposite", w, g, 0))
    case.expect("jac_mul_small on an infinite running sum with the multiplier 2^c - 9, total live",
                lambda m: _has(m, "group.mul_small:inf_running", w, g, (1 << c) - 9) and _has(m, "group.multiple:plus_inf", w, g))
    case.expect("the group's value is 7P", lambda m: m.window_sums[w] == 7 * a % R)
    return case


def case_group_running_cancels_top(c, n, plan):
    """the same inside the top window: digits 15 and 8 of one sub-bucket at c = 12 (indices 100 and 356; the filler partners 256 apart,
    so that the rest of that sub-bucket cancels inside its buckets), plain top digits on the host"""
    a, w = named_log("group-running-top"), n_windows(c) - 1
    if plan == "device":
        assert top_bits(c) == 4
        first, hi, lo = 100, 15, 8
        g, second = (first * 16 + lo) // MSM_GROUP, first + SUB_STRIDE
    else:
        assert top_bits(c) == c
        first, second, hi, lo, g = 0, 1, (1 << c) - 1, (1 << c) - MSM_GROUP, (1 << c) // MSM_GROUP - 1
    placed = {first: (a, digit_scalar(c, {w: hi})), second: (R - a, digit_scalar(c, {w: lo}))}
    case = assemble("group_running_cancels_top", c, n, plan, placed, "apart", 108)
    case.expect("running meets its opposite at digit lo of the top window", lambda m: _has(m, "group.running:opposite", w, g, 0))
    case.expect("jac_mul_small on an infinite running sum (multiplier lo - 1), total live",
                lambda m: _has(m, "group.mul_small:inf_running", w, g, lo - 1) and _has(m, "group.multiple:plus_inf", w, g))
    case.expect("the top window's sum is 7P", lambda m: m.window_sums[w] == 7 * a % R)
    return case


def case_tree(c, n, plan):
    """window 2: groups 0 and 1 both 6P ((P, digit 6) next to ([6 / 8]P, digit 8)); window 4: 6Q and -6Q, then a live group 2"""
    a, b, t = named_log("tree-a"), named_log("tree-b"), named_log("tree-t")
    f = 6 * pow(8, -1, R) % R
    placed = {0: (a, digit_scalar(c, {2: 6})), 1: (a * f, digit_scalar(c, {2: 8})),
              2: (b, digit_scalar(c, {4: 6})), 3: (R - b * f % R, digit_scalar(c, {4: 8})), 4: (t, digit_scalar(c, {4: 20}))}
    case = assemble("tree_equal_opposite", c, n, plan, placed, "apart", 109)
    case.expect("two neighbouring group rows with equal values", lambda m: _has(m, "tree:equal", 2, 0, 0, 1))
    case.expect("two with opposite values, and the chain carries on from infinity", lambda m: _has(m, "tree:opposite", 4, 0, 0, 1) and _has(m, "tree:reborn", 4, 0, 0, 2))
    return case


def case_horner(c, n, plan, start, order):
    """top = the top window or the middle one; S_top = P; then S_w = +-[2^c] acc at the next two windows and live windows below.
    "double_cancel": the first addition must double, the second gives infinity; "cancel_double": the other way round."""
    a, q = named_log("horner-a"), named_log("horner-q")
    W = n_windows(c)
    t = W - 1 if start == "top" else W // 2
    sh = pow(2, c, R)
    inv = lambda d: pow(d, -1, R)
    if order == "double_cancel":
        acc = a * sh * 2 % R                                        # after window t - 1: [2^c]P + [2^c]P
        placed = {0: (a, digit_scalar(c, {t: 1})), 1: (a * sh * inv(5), digit_scalar(c, {t - 1: 5})),
                  2: (R - acc * sh * inv(3) % R, digit_scalar(c, {t - 2: 3})), 3: (q, digit_scalar(c, {t - 4: 9}))}
        want = [("horner:equal", t - 1), ("horner:opposite", t - 2), ("horner:dbl_inf", t - 3), ("horner:reborn", t - 4)]
    else:
        placed = {0: (a, digit_scalar(c, {t: 1})), 1: (R - a * sh * inv(5) % R, digit_scalar(c, {t - 1: 5})),
                  2: (q, digit_scalar(c, {t - 2: 7})), 3: (7 * q * sh * inv(11), digit_scalar(c, {t - 3: 11}))}
        want = [("horner:opposite", t - 1), ("horner:dbl_inf", t - 2), ("horner:reborn", t - 2), ("horner:equal", t - 3)]
    case = assemble("horner_%s_%s" % (start, order), c, n, plan, placed, "adjacent", 110)
    for name, w in want:
        case.expect("%s at the step into window %d" % (name, w), lambda m, name=name, w=w: _has(m, name, w))
    case.expect("live windows below: the sum is not infinity", lambda m: m.result != 0)
    return case


def case_top_digits_only(c, n, plan):
    """k_i = d_i 2^252, d_i in 1..15: on the device (c = 12) every entry lies in the partial top window"""
    P = pool()
    rng = np.random.default_rng(111)
    K = np.zeros((n, 32), dtype=np.uint8)
    K[:, 31] = rng.integers(1, 16, size=n).astype(np.uint8) << 4
    case = Case("top_digits_only", c, plan, P[:n], np.zeros(n, dtype=bool), np.arange(n), K)
    first = 252 // c
    case.expect("every window below bit 252 is empty", lambda m: all(m.used_buckets[w] == 0 and m.window_sums[w] == 0 for w in range(first)))
    case.expect("the top window is live and Horner doubles it down through empty windows", lambda m: m.window_sums[-1] != 0 and m.result != 0)
    return case


BUILDERS = {
    "one_base": case_one_base,
    "p_and_minus_p": case_p_and_minus_p,
    "pairs_only_adjacent": lambda c, n, plan: case_pairs_only(c, n, plan, "adjacent"),
    "pairs_only_apart": lambda c, n, plan: case_pairs_only(c, n, plan, "apart"),
    "pairs_plus_lone": case_pairs_plus_lone,
    "sum_zero_closing": case_sum_zero_closing,
    "group_total_cancels": case_group_total_cancels,
    "group_running_cancels": case_group_running_cancels,
    "group_running_cancels_top": case_group_running_cancels_top,
    "tree_equal_opposite": case_tree,
    "horner_top_double_cancel": lambda c, n, plan: case_horner(c, n, plan, "top", "double_cancel"),
    "horner_top_cancel_double": lambda c, n, plan: case_horner(c, n, plan, "top", "cancel_double"),
    "horner_mid_double_cancel": lambda c, n, plan: case_horner(c, n, plan, "mid", "double_cancel"),
    "top_digits_only": case_top_digits_only,
}


def applies(name, c, plan):
    """top_digits_only leaves the bucket path at c = 16 (fifteen buckets for all terms); the top-window group case needs the 4-bit top
    window on the device and a full one for msm_host's plain digits"""
    if name == "top_digits_only":
        return c != 16
    if name == "group_running_cancels_top":
        return top_bits(c) == 4 if plan == "device" else top_bits(c) == c
    return True


def case_ids(shapes, plan):
    return [(name, c, n) for c, n in shapes for name in BUILDERS if applies(name, c, plan)]


@functools.lru_cache(maxsize=None)
def build(name, c, n, plan="device"):
    """the case (shared, read-only): the same logs and scalars serve G1 and G2 — only base_rows() differs"""
    assert plan == "host" or c == window_bits(n) and n >= MSM_MIN_TERMS
    return BUILDERS[name](c, n, plan)


# ------------------------------------------------------------------------------------------------------------------------- points
_P_LIMBS = [np.uint64((o.P >> (64 * i)) & ((1 << 64) - 1)) for i in range(4)]


def negate_rows(y):
    """p - y on stored residues: uint8 (k, 32 m), each 32-byte little-endian value below p; 0 stays 0"""
    v = np.ascontiguousarray(y).view("<u8").reshape(-1, 4)
    out = np.empty_like(v)
    borrow = np.zeros(v.shape[0], dtype=bool)
    for i in range(4):
        out[:, i] = _P_LIMBS[i] - v[:, i] - borrow.astype(np.uint64)
        borrow = (v[:, i] > _P_LIMBS[i]) | ((v[:, i] == _P_LIMBS[i]) & borrow)
    out[~v.any(axis=1)] = 0
    return out.view(np.uint8).reshape(np.asarray(y).shape)


def log_rows(logs):
    return np.frombuffer(b"".join(a.to_bytes(32, "little") for a in logs), dtype=np.uint8).reshape(-1, 32)


def base_rows(case, width, mul_base, pool_points=None):
    """the bases of a case as uint8 (n, width): mul_base(scalar rows) -> [s]G rows gives the points of the logs (the oracle, or the
    engine's ScalarMultiplicationBase checked against the oracle); pool_points: the rows of pool() when already computed"""
    out = np.zeros((case.n, width), dtype=np.uint8)
    from_pool = case.src >= 0
    if from_pool.any():
        if pool_points is None:
            used = np.unique(case.src[from_pool])
            pts = np.zeros((int(used.max()) + 1, width), dtype=np.uint8)
            pts[used] = np.asarray(mul_base(log_rows([pool()[j] for j in used]))).reshape(-1, width)
            pool_points = pts
        out[from_pool] = pool_points[case.src[from_pool]]
    own = np.flatnonzero(~from_pool)
    distinct = sorted(set(case.logs[i] for i in own))
    pts = np.asarray(mul_base(log_rows(distinct))).reshape(-1, width)
    where = {a: j for j, a in enumerate(distinct)}
    out[own] = pts[[where[case.logs[i]] for i in own]]
    half = width // 2
    out[case.neg, half:] = negate_rows(out[case.neg, half:])
    return out


# -------------------------------------------------------------------------------------------------------------------------- model
def _obj(values):
    a = np.empty(len(values), dtype=object)
    a[:] = values
    return a


def _b(x):
    return np.asarray(x, dtype=bool)


class Model:
    """The plan on integers mod r.  events: name -> int64 array of location rows
         bucket:sum_inf / bucket:all_equal (w, key)        certain in every order of the bucket's members
         bucket:idx_opposite / idx_equal / idx_reborn (w, key)   in ascending index order only
         group.running:K / group.total:K (w, g, j)         at digit lo + j of group g;  K in opposite, equal, reborn
         group.mul_small:inf_running (w, g, lo - 1)        running infinite after having been live, multiplier lo - 1
         group.multiple:K (w, g)                           total + [lo - 1] running;  K as above or plus_inf (multiple infinite, total live)
         tree:K (w, level, t, j)                           the j-th addition of output row t
         horner:K (w) / horner:dbl_inf (w)                 the step into window w (dbl_inf: the c doublings act on infinity that was live)
         result:inf ()
       `reborn`: the accumulator is infinite AFTER having been live and the addend is live — a chain through infinity that carries on.
       window_sums, result: integers mod r;  used_buckets / live_buckets [w]: buckets with members / with a sum other than infinity."""
    def __init__(self, case):
        self._found = {}
        c, plan = case.c, case.plan
        W, nb = n_windows(c), 1 << c
        D = case.keys()
        self.longest = longest_bucket(D, c)
        eff = _obj(case.effective_logs())
        B = self._buckets(D, eff, W, nb)
        self.used_buckets = [int((D[:, w] > 0).any() and np.unique(D[:, w][D[:, w] > 0]).size) for w in range(W)]
        self.live_buckets = [int(_b(B[w] != 0).sum()) for w in range(W)]
        G = self._groups(B, c, W, nb, plan)
        S = self._tree(G, W, plan)
        self.window_sums = [int(s) for s in S]
        self.result = self._horner(self.window_sums, c)
        self.events = {name: np.concatenate(parts) for name, parts in self._found.items()}

    def _rec(self, name, *columns):
        """one location row per element of the columns (equal lengths; no column: one empty row)"""
        rows = np.stack([np.asarray(col, dtype=np.int64).reshape(-1) for col in columns], axis=1) if columns else np.zeros((1, 0), dtype=np.int64)
        if len(rows):
            self._found.setdefault(name, []).append(rows)

    def _classify(self, site, x, y, was_live, loc, active=None, plus_inf=False):
        """x + y elementwise (object arrays of one shape); loc(mask) -> the columns of the location rows"""
        xl, yl = _b(x != 0), _b(y != 0)
        act = np.ones(x.shape, dtype=bool) if active is None else active
        both = xl & yl & act
        self._rec(site + ":opposite", *loc(both & _b((x + y) % R == 0)))
        self._rec(site + ":equal", *loc(both & _b(x == y)))
        self._rec(site + ":reborn", *loc(~xl & was_live & yl & act))
        if plus_inf:
            self._rec(site + ":plus_inf", *loc(xl & ~yl & act))

    def _buckets(self, D, eff, W, nb):
        B = np.zeros((W, nb), dtype=object)
        B[:] = 0
        for w in range(W):
            idx = np.flatnonzero(D[:, w] > 0)
            if not idx.size:
                continue
            order = idx[np.argsort(D[idx, w], kind="stable")]              # by key, ascending index inside a key
            k, v = D[order, w], eff[order]
            start = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
            size = np.diff(np.r_[start, k.size])
            ukey = k[start]
            sums = np.add.reduceat(v, start) % R
            B[w, ukey] = sums
            many = size >= 2
            at = lambda ks: (np.full(len(ks), w), ks)
            self._rec("bucket:sum_inf", *at(ukey[many & _b(sums == 0)]))
            self._rec("bucket:all_equal", *at(ukey[many & _b(np.minimum.reduceat(v, start) == np.maximum.reduceat(v, start))]))
            # ascending index order (what one lane after the other would give): prefix sums inside each bucket
            cs = np.cumsum(v)
            seg = np.repeat(np.arange(start.size), size)
            before = (cs - v - (cs[start] - v[start])[seg]) % R
            first = np.zeros(k.size, dtype=bool); first[start] = True
            live = _b(before != 0)
            self._rec("bucket:idx_opposite", *at(np.unique(k[live & _b((before + v) % R == 0)])))
            self._rec("bucket:idx_equal", *at(np.unique(k[live & _b(before == v)])))
            self._rec("bucket:idx_reborn", *at(np.unique(k[~live & ~first])))
        return B

    def _groups(self, B, c, W, nb, plan):
        """k_msm_groups + msm_group_reduce: group g of window w holds keys [8g, 8g + 8) with weights lo .. lo + 7, lo = 8g & dmask"""
        gpw = nb // MSM_GROUP
        Bg = B.reshape(W, gpw, MSM_GROUP)
        lo = np.tile(np.arange(gpw, dtype=np.int64) * MSM_GROUP, (W, 1))
        tb = top_bits(c)
        if plan == "device" and tb < c:
            lo[W - 1] &= (1 << tb) - 1
        ww, gg = np.meshgrid(np.arange(W), np.arange(gpw), indexing="ij")
        zero = np.zeros((W, gpw), dtype=object); zero[:] = 0
        running, total = zero.copy(), zero.copy()
        run_live, tot_live = np.zeros((W, gpw), dtype=bool), np.zeros((W, gpw), dtype=bool)
        for j in range(MSM_GROUP - 1, -1, -1):
            act = ~((lo == 0) & (j == 0))                                  # the first group starts at digit 1 (lo ? lo : 1u)
            loc = lambda m, j=j: (ww[m], gg[m], np.full(int(m.sum()), j))
            b = Bg[:, :, j]
            self._classify("group.running", running, b, run_live, loc, act)
            running = np.where(act, (running + b) % R, running)
            run_live |= _b(running != 0)
            self._classify("group.total", total, running, tot_live, loc, act)
            total = np.where(act, (total + running) % R, total)
            tot_live |= _b(total != 0)
        mult = lo > 1
        dead = mult & ~_b(running != 0) & run_live
        self._rec("group.mul_small:inf_running", ww[dead], gg[dead], lo[dead] - 1)
        t = np.where(mult, running * (lo - 1).astype(object) % R, zero)
        self._classify("group.multiple", total, t, tot_live, lambda m: (ww[m], gg[m]), mult, plus_inf=True)
        return (total + t) % R

    def _tree(self, G, W, plan):
        """k_msm_rows_sum level by level (fan-in MSM_FAN, the last level what is left); msm_host: one chain over a window's groups"""
        level, per = 0, G.shape[1]
        while per > 1:
            fan = per if plan == "host" else (MSM_FAN if per >= MSM_FAN else per)
            nxt = per // fan
            V = G.reshape(W, nxt, fan)
            ww, tt = np.meshgrid(np.arange(W), np.arange(nxt), indexing="ij")
            acc = np.zeros((W, nxt), dtype=object); acc[:] = 0
            live = np.zeros((W, nxt), dtype=bool)
            for j in range(fan):
                loc = lambda m, j=j: (ww[m], np.full(int(m.sum()), level), tt[m], np.full(int(m.sum()), j))
                self._classify("tree", acc, V[:, :, j], live, loc)
                acc = (acc + V[:, :, j]) % R
                live |= _b(acc != 0)
            G, per, level = acc, nxt, level + 1
        return G.reshape(W)

    def _horner(self, S, c):
        acc = S[-1]
        live = acc != 0
        for w in range(len(S) - 2, -1, -1):
            if acc == 0 and live:
                self._rec("horner:dbl_inf", [w])
            acc = acc * pow(2, c, R) % R
            s = S[w]
            if acc and s:
                if (acc + s) % R == 0:
                    self._rec("horner:opposite", [w])
                if acc == s:
                    self._rec("horner:equal", [w])
            elif s and live:
                self._rec("horner:reborn", [w])
            acc = (acc + s) % R
            live = live or acc != 0
        if acc == 0:
            self._rec("result:inf")
        return acc

    def counts(self):
        return {k: len(v) for k, v in sorted(self.events.items())}


def certify(case, model=None):
    """every event a case is named after, confirmed by the model; and the model's own result equals the exact sum's log (a check of the
    MODEL against the dot product — it is not an expected output for any engine).  Returns the failed texts."""
    m = model or Model(case)
    failed = [text for text, fn in case.checks if not fn(m)]
    if m.result != case.expect_log:
        failed.append("model result != sum of a_i k_i")
    return failed
