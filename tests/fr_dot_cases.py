"""Cases of the segmented inner products in Fr (bn254.fr_dot_segments / fr_sum_segments, csrc/frdot29.hip.hpp), shared by the CPU tests
(tests/test_fr_dot_segments.py, tests/test_fr_dot_bounds.py: the device header on the host) and the GPU tests
(tests/test_fr_dot_segments_gpu.py).  The expectation is Python integers.  The sizes come from the shape constants through the plan of
csrc/segred29.hip.hpp, restated here (pieces, levels): the tests hold the constants against the header and the case list against what
it claims to cover."""
import hashlib

import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
FILL, GROUP, PLAIN_MIN, WAVE = 65536, 512, 512, 64          # FR_DOT_SHAPE and FR_DOT_WAVE
NORM, RUN_MUL, RUN_SUM = 2, 32, 4                          # FR_DOT_NORM, FR_DOT_RUN_MUL, FR_DOT_RUN_SUM
LANES_MIN = 8                                              # FR_DOT_LANES_MIN
ROUND = 2 * WAVE                                           # elements a piece of 64 lanes takes per round
MODES = ("dot", "shared", "sum")


def pieces(n, n_seg, has_k):
    """segred_pieces with FR_DOT_SHAPE"""
    if not n_seg:
        return 1
    by_len = (n // n_seg) // (GROUP if has_k else PLAIN_MIN)
    by_fill = (FILL + n_seg - 1) // n_seg
    return max(min(by_len, by_fill), 1)


def levels(n, n_seg, has_k):
    """[(J, pieces)] per level of segred_levels"""
    out = []
    while True:
        j = pieces(n, n_seg, has_k)
        out.append((j, n_seg * j))
        if j == 1:
            return out
        n, has_k = n_seg * j, False


def piece_lengths(lengths, j):
    """the lengths of the J pieces of every segment (segred_piece_range)"""
    return [[(ln * (p + 1)) // j - (ln * p) // j for p in range(j)] for ln in lengths]


def lanes(n, n_seg, j):
    """fr_dot_lanes: lanes per piece of a launch over n_seg segments of n elements in all, cut in j pieces each"""
    mean = (n // n_seg if n_seg else 0) // j
    L = LANES_MIN
    while L < WAVE and 2 * L < mean:
        L *= 2
    return L


def launch_lanes(n, n_seg, has_k):
    """lanes per piece of every level's launch"""
    out = []
    for j, p in levels(n, n_seg, has_k):
        out.append(lanes(n, n_seg, j))
        n = p
    return out


def rounds(length, L=WAVE):
    return (length + 2 * L - 1) // (2 * L)


def hash_tag(tag):
    return int.from_bytes(hashlib.sha256(tag.encode()).digest()[:8], "little")


def rand_rows(tag, n):
    """n scalar rows with every byte random: values up to 2^256 - 1, most of them above r"""
    return np.random.default_rng(hash_tag(tag)).integers(0, 256, size=(n, 32), dtype=np.uint8)


def const_rows(value, n):
    return np.tile(np.frombuffer(int(value).to_bytes(32, "little"), dtype=np.uint8), (n, 1))


def ints(rows):
    return [int.from_bytes(r.tobytes(), "little") for r in np.asarray(rows, dtype=np.uint8).reshape(-1, 32)]


def rows_of(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32).copy()


def table(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.uint64)


def expect(a, b, seg, n=None, shared=False):
    """out[s] as Python integers -> rows; offsets clamped to n and a shared list ending a segment, as the _dev form reads a table"""
    a, n = ints(a), len(a) if n is None else n
    b = None if b is None else ints(b)
    out = []
    for lo, hi in zip(seg[:-1], seg[1:]):
        lo, hi = min(int(lo), n), min(int(hi), n)
        hi = max(hi, lo)
        if shared and hi - lo > len(b):
            hi = lo + len(b)
        out.append(sum(a[i] * (1 if b is None else b[i - lo] if shared else b[i]) for i in range(lo, hi)) % R)
    return rows_of(out)


# name -> (segment lengths, what the case is there for).  Every case runs in the modes its segments allow (a shared list needs
# segments of one length).
SHORT = [0, 1, 2, 3, 63, 64, 65, 129]
CASES = {
    "short": (SHORT, "segment lengths 0, 1, 2, 3, 63, 64, 65 and 129 in one call"),
    "g_and_g1": ([ROUND, ROUND + 1, ROUND, 2 * ROUND + 1, 2 * ROUND, 1], "64 lanes per piece: neighbouring wavefronts with G and G + 1 rounds"),
    "short_mixed": ([15, 16, 17, 33, 0, 1, 32, 16, 2, 16, 31, 16, 9], "8 lanes per piece: G and G + 1 rounds inside one wavefront, 13 pieces for 16 slots"),
    "one_long_piece": ([RUN_MUL * ROUND * 2 - 300, 0, 0, 0, 0, 0, 0, 0], "J = 1 with a piece that passes a reduction (more than RUN_MUL rounds)"),
    "two_levels": ([2 * GROUP + 1], "one segment cut in two pieces of G and G + 1 rounds: exactly two levels"),
    "cut_uneven": ([3 * GROUP - 36, 0, 4 * GROUP - 100], "three segments, J = 2, an empty one among them"),
    "shared_short": ([130] * 5, "a shared list, no cut"),
    "shared_cut": ([2 * GROUP + 76] * 2, "a shared list over cut segments"),
    "three_levels": ([(1 << 19) + 77], "one segment, three levels"),
}
EXTREMES = {"r_minus_1": R - 1, "all_ones": (1 << 256) - 1, "zero": 0}


def case_modes(lengths):
    uniform = len(set(lengths)) == 1
    return [m for m in MODES if m != "shared" or uniform]


def case_inputs(name, mode):
    """(a rows, b rows or None, table, shared) of a case"""
    lengths = CASES[name][0]
    n = sum(lengths)
    a = rand_rows(name + "/a", n)
    if mode == "sum":
        return a, None, table(lengths), False
    if mode == "shared":
        return a, rand_rows(name + "/b", lengths[0]), table(lengths), True
    return a, rand_rows(name + "/b", n), table(lengths), False


def extreme_inputs(value):
    """the longest run between two reductions with every operand at `value`: the one_long_piece shape"""
    lengths = CASES["one_long_piece"][0]
    n = sum(lengths)
    return const_rows(value, n), const_rows(value, n), table(lengths)
