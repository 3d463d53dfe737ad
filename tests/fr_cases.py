"""Inputs and expectations of the scalar-field tests (tests/test_fr.py on the CPU harness, tests/test_fr_gpu.py on the device):
edge values and seeded random scalars for the elementwise operations, values that are 0 modulo r at every position of an
inversion group, root lists for the two polynomial kernels, and Python's integer arithmetic modulo r as the one expectation
(pow(x, -1, r), afp25.poly_from_roots, afp25.quotient_by_root).  Every comparison is exact.

Run as a script it sends the same kinds of input through the host-pointer entries in a process of its own bound to the device
list given on the command line (a device may be listed twice, so one GPU still crosses the shard split)."""
import os
import sys

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle")]

import numpy as np  # noqa: E402

import bn254_py as o  # noqa: E402
from gopairingbasedcryptography_amd import afp25  # noqa: E402

R = o.R
assert 5 * R < 1 << 256 < 6 * R
EDGES = [0, 1, 2, R - 1, R, R + 1, 2 * R, 5 * R, 1 << 255, (1 << 256) - 1] + [(1 << (29 * k)) + d for k in range(1, 9) for d in (-1, 0, 1)]
ZEROS = [m * R for m in range(6)]                      # every value below 2^256 that is 0 modulo r
MONT = 1 << 256
BINARY = ("add", "sub", "mul")
UNARY = ("neg", "inverse", "from_mont", "to_mont")
OP_CODE = {"add": 0, "sub": 1, "mul": 2, "neg": 3, "from_mont": 4, "to_mont": 5, "inverse": 6}     # FrOp of csrc/fr29.hip.hpp; 6 = FR_OPS
PY = {
    "add": lambda a, b: (a + b) % R, "sub": lambda a, b: (a - b) % R, "mul": lambda a, b: a * b % R, "neg": lambda a, b: -a % R,
    "inverse": lambda a, b: pow(a, -1, R) if a % R else 0,
    "from_mont": lambda a, b: a * pow(MONT, -1, R) % R, "to_mont": lambda a, b: a * MONT % R,
}
SIZES = lambda K: (1, K - 1, K + 1, 1000)
POLY_BS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1024)


def rows(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32).copy()


def ints(buf):
    return [int.from_bytes(r.tobytes(), "little") for r in np.asarray(buf, dtype=np.uint8).reshape(-1, 32)]


def rand(tag, n):
    return [o.bench_scalar("fr-" + tag, i) for i in range(n)]


def expect(op, A, B=None):
    """Python's result row by row (B of one value: broadcast)"""
    return [PY[op](a, None if B is None else B[i if len(B) > 1 else 0]) for i, a in enumerate(A)]


def zero_batch(K, z, tag):
    """K + 1 inversion lanes of K elements (T = K + 1, n = K (K + 1)): lane t < K has the value z (0 modulo r) at position t of its
    group (element t + t T), lane K is made of nothing else"""
    T = K + 1
    A = rand(tag, K * T)
    for i in [t + t * T for t in range(K)] + [K + j * T for j in range(K)]:
        A[i] = z
    return A


def elementwise_cases(K):
    """(label, op, A, B): B is None for the unary operations and one value for a broadcast"""
    out = []
    pairs_a = [x for x in EDGES for _ in EDGES]
    pairs_b = [y for _ in EDGES for y in EDGES]
    for op in BINARY:
        out.append(("edges", op, pairs_a, pairs_b))
        for n in SIZES(K):
            out.append(("rand%d" % n, op, rand("a-%s-%d" % (op, n), n), rand("b-%s-%d" % (op, n), n)))
        for j, b in enumerate((rand("bc-" + op, 1)[0], 0, R, (1 << 256) - 1)):
            out.append(("broadcast%d" % j, op, EDGES + rand("bca-%s-%d" % (op, j), 5 * K + 3), [b]))
    for op in UNARY:
        out.append(("edges", op, list(EDGES), None))
        for n in SIZES(K):
            out.append(("rand%d" % n, op, rand("u-%s-%d" % (op, n), n), None))
    for z in ZEROS:
        out.append(("zero%d" % (z // R), "inverse", zero_batch(K, z, "z%d" % (z // R)), None))
    mixed = rand("zmix", 3 * K + 1)
    for i, z in enumerate(ZEROS):
        mixed[(2 * i + 1) % len(mixed)] = z
    out.append(("zeros-mixed", "inverse", mixed, None))
    return out


# ------------------------------------------------------------------------------------------------ polynomials
def poly_cases(B):
    """root lists (k polynomials of B roots) holding root 0, a repeated root, roots >= r and 2^256 - 1 as far as B has room"""
    a, b, c = rand("pa-%d" % B, B), rand("pb-%d" % B, B), rand("pc-%d" % B, B)
    a[0] = 0
    if B >= 3:
        a[2] = a[1]
    b[-1] = R + 5
    if B >= 2:
        b[0] = (1 << 256) - 1
        c = [c[0]] * 2 + c[2:]
    if B >= 4:
        c[3] = c[0] + R                                 # the repeated root once more, unreduced
    return [a, b, c]


def non_root(roots):
    v = 7
    while any((v - x) % R == 0 for x in roots):
        v += 1
    return v


def quotient_case(polys, B):
    """(coefficient rows [k][B + 1], points [k][B], expected rows [k*B][B] or None where the point is no root).  Polynomial 0 gets a
    non-root in the middle and, from B = 3 on, at its last point."""
    coeffs = [afp25.poly_from_roots(p) for p in polys]
    points = [list(p) for p in polys]
    points[0][B // 2] = non_root(polys[0])
    if B >= 3:
        points[0][B - 1] = non_root(polys[0]) + R
    want = []
    for j, p in enumerate(polys):
        for i, x in enumerate(points[j]):
            want.append(afp25.quotient_by_root(coeffs[j], x) if any((x - y) % R == 0 for y in p) else None)
    return coeffs, points, want


def check_quotients(q, ok, want, B, stride):
    """q: [k*B, stride, 32] rows, ok: [k*B]; returns the list of rows that differ from `want`"""
    q = np.asarray(q).reshape(len(want), stride, 32)
    bad = []
    for r, w in enumerate(want):
        exp = rows((w if w is not None else [0] * B) + [0] * (stride - B))
        if int(ok[r]) != (w is not None) or not (q[r] == exp).all():
            bad.append(r)
    return bad


def others_product_matches(polys, want, B, every=1):
    """the quotient for root i equals prod over the OTHER roots (what the reference's Decrypt multiplies out), for every `every`-th row"""
    for j, p in enumerate(polys):
        for i in range(0, B, every):
            w = want[j * B + i]
            if w is not None and w != afp25.poly_from_roots(p[:i] + p[i + 1:]):
                return (j, i)
    return None


# ------------------------------------------------------------------------------------------------ the engine's entries
def run_engine_cases(eng, K, dev=None, in_place=True):
    """every elementwise case through eng.fr_* (host arrays, or CUDA tensors when `dev` moves an array to the device); out = a and,
    with one b per a, out = b as well.  Returns the list of failures."""
    bad = []
    back = (lambda x: x) if dev is None else (lambda x: x.cpu().numpy())
    put = (lambda x: x) if dev is None else dev
    for label, op, A, B in elementwise_cases(K):
        want = rows(expect(op, A, B))
        f = getattr(eng, "fr_" + op)
        a = put(rows(A))
        args = (a,) if B is None else (a, put(rows(B)))
        if not (back(f(*args)).reshape(-1, 32) == want).all():
            bad.append((label, op))
        if in_place:
            a2 = put(rows(A))
            f(*((a2,) + args[1:]), out=a2)
            if not (back(a2).reshape(-1, 32) == want).all():
                bad.append((label, op, "out=a"))
            if B is not None and len(B) == len(A):
                b2 = put(rows(B))
                f(a, b2, out=b2)
                if not (back(b2).reshape(-1, 32) == want).all():
                    bad.append((label, op, "out=b"))
    return bad


def run_engine_poly(eng, Bs, dev=None):
    bad = []
    back = (lambda x: x) if dev is None else (lambda x: x.cpu().numpy())
    put = (lambda x: x) if dev is None else dev
    for B in Bs:
        polys = poly_cases(B)
        got = back(eng.fr_poly_from_roots(put(rows([x for p in polys for x in p]).reshape(-1)), B))
        coeffs, points, want = quotient_case(polys, B)
        if ints(got) != [c for f in coeffs for c in f]:
            bad.append(("from_roots", B))
        for stride in (B, B + 1, B + 7):
            q, ok = eng.fr_poly_quotients(put(rows([c for f in coeffs for c in f]).reshape(-1)), put(rows([x for p in points for x in p]).reshape(-1)), B, stride)
            wrong = check_quotients(back(q), back(ok), want, B, stride)
            if wrong:
                bad.append(("quotients", B, stride, wrong[:8]))
    return bad


def shard_run(eng):
    """host-pointer entries on batches large enough for the shard split (elementwise: 2 x 16384 elements; polynomials: 2 x
    max(1, 2^16 / B^2) of them) plus the case lists on the smaller routes"""
    bad = run_engine_cases(eng, 8) + run_engine_poly(eng, (3, 64, 256))
    n = 40000
    A, B = rand("shard-a", n), rand("shard-b", n)
    for i, e in enumerate(EDGES):
        A[(i * 1237) % n] = e
        B[(i * 2311 + 20000) % n] = e
    for z in ZEROS:
        A[n // 2 - 3 + z // R] = z
    for op in BINARY + UNARY:
        got = getattr(eng, "fr_" + op)(*((rows(A), rows(B)) if op in BINARY else (rows(A),)))
        if not (got == rows(expect(op, A, B if op in BINARY else None))).all():
            bad.append(("shard", op))
    for Bp, k in ((3, 15000), (64, 40), (256, 3)):
        roots = [rand("shard-p%d-%d" % (Bp, j), Bp) for j in range(k)] if Bp > 3 else np.array(rand("shard-p3", 3 * k), dtype=object).reshape(k, 3).tolist()
        got = eng.fr_poly_from_roots(roots)
        coeffs = [afp25.poly_from_roots(p) for p in roots]
        if ints(got) != [c for f in coeffs for c in f]:
            bad.append(("shard from_roots", Bp))
        q, ok = eng.fr_poly_quotients(got.reshape(-1), rows([x for p in roots for x in p]).reshape(-1), Bp, Bp + 1)
        want = [afp25.quotient_by_root(coeffs[j], x) for j, p in enumerate(roots) for x in p]
        if check_quotients(q, ok, want, Bp, Bp + 1):
            bad.append(("shard quotients", Bp))
    return bad


if __name__ == "__main__":
    # python fr_cases.py DEV [DEV ...]
    from gopairingbasedcryptography_amd import bn254 as engine
    engine.init([int(d) for d in sys.argv[1:]])
    failures = shard_run(engine)
    print("devices", engine.num_devices(), "failures", failures)
    sys.exit(1 if failures else 0)
