"""Cases of the group-law tests (tests/test_group_law.py on the CPU harness, tests/test_group_law_gpu.py on the device): points
from seeded scalars, the oracle's expectation row by row, special cases placed at given positions of the inversion groups, and
the 2^20 algebraic check against the engine's scalar multiplication.  Run as a script it performs that check through the
host-pointer entries in a process of its own bound to the device list given on the command line (a device may be listed
twice, so one GPU still crosses the shard split)."""
import os
import sys

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle")]

import numpy as np  # noqa: E402

import bn254_py as o  # noqa: E402

ADD, SUB, DBL = 0, 1, 2
OPS = (ADD, SUB, DBL)


# ------------------------------------------------------------------------------------------------ points and expectations
class Group:
    def __init__(self, g2):
        self.g2 = g2
        self.width = 128 if g2 else 64
        self.add = o.g2_add if g2 else o.g1_add
        self.neg = o.g2_neg if g2 else o.g1_neg
        self.to_bytes = o.g2_to_bytes if g2 else o.g1_to_bytes
        self.from_bytes = o.g2_from_bytes if g2 else o.g1_from_bytes
        self.gen = o.G2_GEN if g2 else o.G1_GEN

    def points(self, oracle, tag, n):
        """n points [k_i] gen for seeded scalars k_i (the C oracle's scalar multiplication), as an (n, width) uint8 array"""
        k = np.frombuffer(b"".join(o.scalar_to_bytes(o.bench_scalar(tag, i)) for i in range(n)), dtype=np.uint8).copy()
        mul = oracle.g2_scalar_mul if self.g2 else oracle.g1_scalar_mul
        return np.asarray(mul(np.frombuffer(self.to_bytes(self.gen), dtype=np.uint8), k)).reshape(n, self.width).copy()

    def neg_rows(self, rows):
        return np.frombuffer(b"".join(self.to_bytes(self.neg(self.from_bytes(r.tobytes()))) for r in rows), dtype=np.uint8).reshape(-1, self.width).copy()

    def expect(self, op, A, B):
        """the oracle's a OP b row by row (B of one row: broadcast)"""
        out = []
        for i in range(A.shape[0]):
            a = self.from_bytes(A[i].tobytes())
            if op == DBL:
                r = self.add(a, a)
            else:
                b = self.from_bytes(B[i if B.shape[0] > 1 else 0].tobytes())
                r = self.add(a, b if op == ADD else self.neg(b))
            out.append(self.to_bytes(r))
        return np.frombuffer(b"".join(out), dtype=np.uint8).reshape(-1, self.width)


GROUPS = {"g1": Group(False), "g2": Group(True)}
SPECIALS = ("a_inf", "b_inf", "both_inf", "a_eq_b", "a_eq_neg_b")


def make_special(grp, kind, A, B, i):
    """element i of (A, B) becomes the special case `kind` (for SUB, a_eq_b is a - a and a_eq_neg_b is a doubling)"""
    if kind in ("a_inf", "both_inf"):
        A[i] = 0
    if kind in ("b_inf", "both_inf"):
        B[i] = 0
    if kind == "a_eq_b":
        B[i] = A[i]
    if kind == "a_eq_neg_b":
        B[i] = grp.neg_rows(A[i:i + 1])[0]


def special_batch(grp, oracle, op, kind, K, tag):
    """K + 1 lanes of K elements (T = K + 1, n = K (K + 1)): lane t < K has the special case at position t of its inversion
    group (element t + t T), lane K has it at every position"""
    T = K + 1
    n = K * T
    A, B = grp.points(oracle, tag + "a", n), grp.points(oracle, tag + "b", n)
    idx = [t + t * T for t in range(K)] + [K + j * T for j in range(K)]
    for i in idx:
        make_special(grp, kind, A, B, i)
    return A, B


def run_hc(hc, grp, op, A, B, k=0):
    n = A.shape[0]
    A = np.ascontiguousarray(A)
    Bc = np.ascontiguousarray(A if B is None else B)
    nb = n if B is None else Bc.shape[0]
    out = np.zeros((n, grp.width), dtype=np.uint8)
    rc = hc.hc_group_op(1 if grp.g2 else 0, op, A.ctypes.data, Bc.ctypes.data, nb, n, out.ctypes.data, k)
    assert rc == 0
    return out


def group_k(hc, grp):
    """elements per shared inversion in the kernels of this group"""
    return int(hc.hc_group_k(1 if grp.g2 else 0))


# ------------------------------------------------------------------------------------------------ the 2^20 algebraic check
SPECIAL_SCALARS = ("a0", "b0", "both0", "b=a", "b=-a")


def special_positions(n, K, wave=64):
    """indices at the edges of inversion groups (lane t owns t + j T, T = ceil(n / K)), of wavefronts (= workgroups: one wave
    each) and of the two-way shard split"""
    T = (n + K - 1) // K
    idx = set()
    for j in range(K):
        for off in (0, 1, wave - 1, wave, wave + 1, T - 2, T - 1):
            idx.add(j * T + off)
    for m in (n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1, 1000 * wave - 1, 1000 * wave):
        idx.add(m)
    return sorted(i for i in idx if 0 <= i < n)


def algebraic_scalars(n, K, seed):
    """(a, b) as Python ints mod r and their 32-byte rows, with a = 0, b = 0, both 0, b = a and b = -a at special_positions;
    also the rows of a + b, a - b and 2a (mod r).  Returns (positions, rows dict)."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 1 << 32, size=(2, n, 8), dtype=np.uint64).astype(np.uint32)
    raw[:, :, 7] &= 0x1FFFFFFF                                      # < 2^253 < r
    a = [int.from_bytes(raw[0, i].tobytes(), "little") for i in range(n)]
    b = [int.from_bytes(raw[1, i].tobytes(), "little") for i in range(n)]
    pos = special_positions(n, K)
    for c, i in enumerate(pos):
        kind = SPECIAL_SCALARS[c % len(SPECIAL_SCALARS)]
        if kind in ("a0", "both0"):
            a[i] = 0
        if kind in ("b0", "both0"):
            b[i] = 0
        if kind == "b=a":
            b[i] = a[i]
        if kind == "b=-a":
            b[i] = (o.R - a[i]) % o.R
    rows = lambda ks: np.frombuffer(b"".join(k.to_bytes(32, "little") for k in ks), dtype=np.uint8).reshape(n, 32).copy()
    return pos, {"a": rows(a), "b": rows(b), "sum": rows([(x + y) % o.R for x, y in zip(a, b)]),
                 "diff": rows([(x - y) % o.R for x, y in zip(a, b)]), "dbl": rows([2 * x % o.R for x in a])}


def host_check(eng, g2, pts, lane_units=16384):
    """the host-pointer entries on the whole batch and on one slice of lane_units elements around the middle (the own-lane route);
    pts: numpy rows of A, B and the expected A + B, A - B, 2A.  Returns a list of failures."""
    add, sub, dbl = (eng.g2_add, eng.g2_sub, eng.g2_double) if g2 else (eng.g1_add, eng.g1_sub, eng.g1_double)
    A, B = pts["A"], pts["B"]
    bad = []
    n = A.shape[0]
    for name, got, want in (("add", add(A, B), pts["sum"]), ("sub", sub(A, B), pts["diff"]), ("dbl", dbl(A), pts["dbl"])):
        wrong = np.nonzero((got != want).any(axis=1))[0]
        if wrong.size:
            bad.append(("host", name, wrong[:8].tolist(), int(wrong.size)))
    lo = n // 2 - lane_units // 2
    s = slice(lo, lo + lane_units)
    for name, got, want in (("add", add(A[s], B[s]), pts["sum"][s]), ("sub", sub(A[s], B[s]), pts["diff"][s]), ("dbl", dbl(A[s]), pts["dbl"][s])):
        wrong = np.nonzero((got != want).any(axis=1))[0]
        if wrong.size:
            bad.append(("lane", name, wrong[:8].tolist(), int(wrong.size)))
    return bad


if __name__ == "__main__":
    # python group_law_cases.py IN.npz g1|g2 DEV [DEV ...]: the host-pointer entries over the given device list on the rows of IN.npz
    from gopairingbasedcryptography_amd import bn254 as eng
    eng.init([int(d) for d in sys.argv[3:]])
    data = np.load(sys.argv[1])
    failures = host_check(eng, sys.argv[2] == "g2", {k: data[k] for k in ("A", "B", "sum", "diff", "dbl")})
    print("devices", eng.num_devices(), "failures", failures)
    sys.exit(1 if failures else 0)
