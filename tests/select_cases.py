"""Cases for the common attributes of a list and a set (csrc/select29.hip.hpp, include/gpbc_bn254_select.h), shared by the CPU and the
GPU tests: a case list and expected(case), utils/find_common_attributes.go restated in Python integers with the positions
sw05.select_common defines.  Nothing here shares code with the kernel.

A case: label, m, a, d, k, shared, sets ([1][m] or [k][m] integers below 2^256) and lists ([k][a]).  The shapes are the smallest at which
the kernel can go wrong: a on both sides of a wave and of a chunk (1, 2, 31 .. 33, 63 .. 65, 129), m on both sides of the staging loop
and of the small LDS instance (1, 2, 63 .. 65, 257), k with a last workgroup that is not full (1, 3, 65, 130), a set for all items and a
set per item, and the limit m = a = d = 1024."""
import functools
import random

import numpy as np

import bn254_py as o

R = o.R
TOP = (1 << 256) - 1
A_SIZES, M_SIZES, K_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 129), (1, 2, 63, 64, 65, 257), (1, 3, 65, 130)
NAMED = (0, 1, R - 1, R, R + 20, 5 * R + 3, TOP)


def rows(values):
    """integers below 2^256 as 32-byte little-endian rows, unreduced: [n, 32] uint8"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32).copy()


def set_rows(case):
    return rows(v for s in case["sets"] for v in s)


def list_rows(case):
    return rows(v for lst in case["lists"] for v in lst)


def item_set(case, j):
    return case["sets"][0 if case["shared"] else j]


def expected_item(S, L, d):
    """FindCommonAttributes(S, L, d) with positions: [(set position, list position, value mod r)] of the first d kept, or None"""
    first = {}
    for p, v in enumerate(S):
        first.setdefault(v % R, p)
    seen, kept = set(), []
    for p, v in enumerate(L):
        c = v % R
        if c in first and c not in seen:
            seen.add(c)
            kept.append((first[c], p, c))
    return kept[:d] if len(kept) >= d else None


def expected(case):
    """(set_pos [k, d] uint32, list_pos [k, d] uint32, common [k, d, 32] uint8, ok [k] uint8)"""
    k, d = case["k"], case["d"]
    sp, lp = np.zeros((k, d), dtype=np.uint32), np.zeros((k, d), dtype=np.uint32)
    common, ok = np.zeros((k, d, 32), dtype=np.uint8), np.zeros(k, dtype=np.uint8)
    for j in range(k):
        kept = expected_item(item_set(case, j), case["lists"][j], d)
        if kept is not None:
            sp[j], lp[j], ok[j] = [t[0] for t in kept], [t[1] for t in kept], 1
            common[j] = rows(t[2] for t in kept)
    return sp, lp, common, ok


def mismatches(case, got):
    """what differs between a result (set_pos, list_pos, common, ok — any integer / byte arrays of the right sizes) and expected(case)"""
    k, d = case["k"], case["d"]
    want = expected(case)
    bad = []
    for name, g, w, shape in zip(("set_pos", "list_pos", "common", "ok"), got, want, ((k, d), (k, d), (k, d, 32), (k,))):
        g = np.asarray(g).reshape(shape)
        if not np.array_equal(g.astype(np.int64), w.astype(np.int64)):
            rows_bad = np.nonzero((g.astype(np.int64) != w.astype(np.int64)).reshape(k, -1).any(1))[0]
            bad.append("%s: %s differs for items %s" % (case["label"], name, rows_bad[:8].tolist()))
    return bad


# ------------------------------------------------------------------------------------------------ building items
def variants(c):
    """the representatives of the residue c below 2^256"""
    return [c + t * R for t in range(6) if c + t * R <= TOP]


def _residues(rng, n, avoid=()):
    out, have = [], set(avoid)
    pool = [v % R for v in NAMED] + [3, 20]
    rng.shuffle(pool)
    while len(out) < n:
        c = pool.pop() if pool and rng.random() < 0.5 else rng.randrange(R)
        if c not in have:
            have.add(c)
            out.append(c)
    return out


def make_set(rng, m):
    """m values over m - (0 .. 2) distinct residues: repeats sit at random places, any representative of a residue"""
    distinct = _residues(rng, max(1, m - rng.randrange(0, min(3, m))))
    res = distinct + [rng.choice(distinct) for _ in range(m - len(distinct))]
    rng.shuffle(res)
    return [rng.choice(variants(c)) for c in res]


def make_list(rng, S, a, d, mode):
    """a values of which `mode` decides how many distinct residues the set holds: 'exact' d with the d-th at the last position, 'short'
    d - 1, 'more' more than d, 'any' a random number; the rest are repeats of those (as bytes or only modulo r) and values the set does not
    hold, among them neighbours of set elements that differ in the lowest or in the highest word only"""
    held = list(dict.fromkeys(v % R for v in S))
    cap = min(len(held), a)
    want = {"exact": d, "short": d - 1, "more": d + 1 + rng.randrange(3), "any": rng.randint(0, cap)}[mode]
    c = max(0, min(want, cap))
    common = rng.sample(held, c)
    fill = a - c
    last = common[-1] if mode == "exact" and c == d else None
    front = common[:-1] if last is not None else common
    body = [rng.choice(variants(v)) for v in front]
    n_rep = rng.randrange(0, fill // 2 + 1) if front else 0
    reps = [rng.choice(variants(rng.choice(front))) for _ in range(n_rep)]
    others, have = [], set(held)
    while len(others) < fill - n_rep:
        base = rng.choice(S)
        cand = rng.choice([base ^ 1, base ^ (1 << 230), rng.randrange(1 << 256), rng.randrange(R)]) & TOP
        if cand % R not in have:
            others.append(cand)
    body += reps + others
    rng.shuffle(body)
    if last is not None:
        body.append(rng.choice(variants(last)))
    assert len(body) == a
    return body


def make_case(label, seed, m, a, d, k, shared):
    rng = random.Random(seed)
    sets = [make_set(rng, m) for _ in range(1 if shared else k)]
    modes = ["exact", "short", "more", "any"]
    lists = [make_list(rng, sets[0 if shared else j], a, d, modes[(j + seed) % 4]) for j in range(k)]
    return dict(label=label, m=m, a=a, d=d, k=k, shared=shared, sets=sets, lists=lists)


# ------------------------------------------------------------------------------------------------ written out by hand
def reference_table(d):
    """the six ciphertexts of test_sw05_plan.py::test_select_common_follows_the_reference_rule; rows are rectangular here, so the lists of
    five are filled up to seven with values the key does not hold, which changes nothing"""
    key = [7, 3, 11, 5, 3, R + 20]
    cts = [[5, 9, 3, 7, 11], [9, 3, 3, 8, 3 + R, 11, 7], [11, 9, 8, 7, 3], [11, 9, 8, 7, 4], [20, 1, 2, 5, 7], [1, 2, 4, 6, 8]]
    return dict(label="reference-table/d%d" % d, m=6, a=7, d=d, k=6, shared=True, sets=[key], lists=[c + [100, 101][:7 - len(c)] for c in cts])


def named_values():
    """0, 1, r - 1, r, r + 20, 5 r + 3 and 2^256 - 1 on either side; the set holds v + r where the list holds v; 7 twice in the set"""
    S = [R + 20, 1, R - 1, 5 * R + 3, TOP, 7, 7 + R, 0]
    lists = [[R, 20, 1, TOP, 3, R - 1],                       # r is 0 (position 7), 20 is r + 20, 3 is 5 r + 3: four kept before r - 1
             [7 + R, 7, 7 + 2 * R, 2, 4, 7],                  # one residue four times: one kept
             [TOP % R, 2 * R - 1, R + 1, 0, 5 * R + 3, 2 * R + 20],      # every one equal to a set element only modulo r
             [2, 4, 5 * R + 4, R - 2, TOP - 1, R + 2]]        # neighbours of set elements: nothing
    return dict(label="named-values", m=8, a=6, d=4, k=4, shared=True, sets=[S], lists=lists)


def word_pairs():
    """values that differ in the lowest word only, or in the highest word only, on both sides"""
    x, y = o.bench_scalar("select-x", 0) % (1 << 250), o.bench_scalar("select-y", 0) % (1 << 250)
    S = [x, x ^ 1, y, y ^ (1 << 250), x ^ (1 << 32)]
    lists = [[x ^ 1, y ^ (1 << 250), x ^ 2, y ^ (1 << 249), x], [y ^ (1 << 251), x ^ 3, y ^ 1, x ^ (1 << 32), y], [x ^ (1 << 224), y ^ (1 << 224), x ^ (1 << 31), y ^ 2, x ^ 4]]
    return dict(label="word-pairs", m=5, a=5, d=2, k=3, shared=True, sets=[S], lists=lists)


def chunked():
    """a = 129: a repeat whose first occurrence lies in an earlier chunk, kept elements on both sides of a chunk boundary, the d-th kept
    element at the last list position, per item sets"""
    rng = random.Random(129)
    items = []
    for j in range(3):
        S = make_set(rng, 65)
        held = list(dict.fromkeys(v % R for v in S))
        out = lambda: next(v for v in iter(lambda: rng.randrange(1 << 256), None) if v % R not in set(held))
        L = [out() for _ in range(129)]
        c = held[:6]
        if j == 0:                                            # kept at 3, 62, 63 | 64, 65, 128; repeats of 3 and 63 at 70 (bytes) and 127 (mod r)
            for p, v in zip((3, 62, 63, 64, 65, 128), c):
                L[p] = v
            L[70], L[127] = c[0], c[2] + R
        elif j == 1:                                          # four only, none in the first chunk
            for p, v in zip((64, 100, 127, 128), c):
                L[p] = v
            L[126] = c[0] + R
        else:                                                 # five only
            for p, v in zip((0, 63, 64, 127, 128), c):
                L[p] = v
            L[65], L[66] = c[0], c[1]
        items.append((S, L))
    return dict(label="chunked", m=65, a=129, d=6, k=3, shared=False, sets=[s for s, _ in items], lists=[l for _, l in items])


def limit_cases():
    rng = random.Random(1024)
    S = _residues(rng, 1024)
    perm = S[:]
    rng.shuffle(perm)
    broken = perm[:]
    broken[517] = next(v for v in iter(lambda: rng.randrange(R), None) if v not in set(S))
    full = dict(label="limit/1024-of-1024", m=1024, a=1024, d=1024, k=2, shared=True, sets=[S], lists=[perm, broken])
    others = _residues(rng, 2046, avoid=S[-1:])
    last = dict(label="limit/last-to-last", m=1024, a=1024, d=1, k=1, shared=True, sets=[others[:1023] + [S[-1] + R]], lists=[others[1023:] + [S[-1]]])
    return [full, last]


@functools.lru_cache(maxsize=None)
def cases():
    out = [reference_table(1), reference_table(3), reference_table(4), named_values(), word_pairs(), chunked()] + limit_cases()
    n = 0
    for ai, a in enumerate(A_SIZES):
        for mi, m in enumerate(M_SIZES):
            k = K_SIZES[(ai + mi) % 4]
            shared = (ai + 2 * mi + n) % 2 == 0
            lo = min(a, m)
            d = (1, max(1, lo // 2), lo, max(1, lo - 1))[(ai + mi * 2) % 4]
            out.append(make_case("a%d-m%d-k%d-%s" % (a, m, k, "shared" if shared else "own"), 1000 + n, m, a, d, k, shared))
            n += 1
    # every k and both kinds of set at one shape that fills a wave unevenly, and d beyond the list and beyond the set
    for k in K_SIZES:
        for shared in (True, False):
            out.append(make_case("a24-m32-k%d-%s" % (k, "shared" if shared else "own"), 2000 + k + shared, 32, 24, 16, k, shared))
    out.append(make_case("d-beyond-a", 3001, 64, 3, 4, 3, True))
    out.append(make_case("d-beyond-m", 3002, 2, 33, 3, 65, False))
    assert len({c["label"] for c in out}) == len(out)
    return tuple(out)


def by_label(label):
    return next(c for c in cases() if c["label"] == label)


def classes(case):
    """the classes of the issue's list that a case contains, found from the integers alone"""
    found = set()
    m, a, d, k = case["m"], case["a"], case["d"], case["k"]
    if d > a:
        found.add("d > a")
    if d > m:
        found.add("d > m")
    for j in range(k):
        S, L = item_set(case, j), case["lists"][j]
        for v in list(S) + list(L):
            if v in NAMED:
                found.add("value %d" % NAMED.index(v))
        first = {}
        for p, v in enumerate(S):
            first.setdefault(v % R, p)
        where = {}
        for p, v in enumerate(L):
            if v % R in first:
                where.setdefault(v % R, []).append(p)
        for c, ps in where.items():
            if len(ps) > 1:
                found.add("list repeat as bytes" if any(L[p] == L[ps[0]] for p in ps[1:]) else "list repeat modulo r only")
                if any(L[p] != L[ps[0]] for p in ps[1:]):
                    found.add("list repeat modulo r only")
                if ps[0] < 64 <= ps[-1]:
                    found.add("repeat of an earlier chunk's element")
            if sum(1 for v in S if v % R == c) > 1:
                found.add("set repeat that the list holds")
            if L[ps[0]] + R == S[first[c]]:
                found.add("set holds v + r, list holds v")
        n_common = len(where)
        kept = expected_item(S, L, d)
        if n_common == d and kept and kept[-1][1] == a - 1:
            found.add("exactly d, the last at the end of the list")
        if n_common == d - 1:
            found.add("d - 1 common")
        if n_common > d:
            found.add("more than d common")
        if kept and any(t[1] < 64 for t in kept) and any(t[1] >= 64 for t in kept):
            found.add("kept elements on both sides of a chunk boundary")
        for vals in (S, L):
            for i, u in enumerate(vals):
                for v in vals[i + 1:i + 8]:
                    x = u ^ v
                    if x and x < (1 << 32):
                        found.add("pair that differs in the lowest word")
                    if x and not x & ((1 << 224) - 1):
                        found.add("pair that differs in the highest word")
    return found


CLASSES = {"d > a", "d > m", "list repeat as bytes", "list repeat modulo r only", "repeat of an earlier chunk's element", "set repeat that the list holds",
           "set holds v + r, list holds v", "exactly d, the last at the end of the list", "d - 1 common", "more than d common",
           "kept elements on both sides of a chunk boundary", "pair that differs in the lowest word", "pair that differs in the highest word"} | {
               "value %d" % i for i in range(len(NAMED))}
