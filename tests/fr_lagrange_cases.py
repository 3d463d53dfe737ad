"""Inputs and expectations of the Lagrange-basis tests (tests/test_fr_lagrange.py on the CPU harness, tests/test_fr_lagrange_gpu.py
on the device).  The expectation is Python's integer arithmetic modulo r: `basis` multiplies numerator and denominator out and
inverts once per output, `basis_reference_loop` is utils.ComputeLagrangeBasis as the reference writes it (one inversion per factor).

A case is a dict: set [ns][B], nodes [nn][m] or None (the set's own elements), x [nx] or None (evaluate at 0), k rows; ns and nn
are 1 or k, nx is 1 or k.  `run_cases(call, cases)` sends each through call(set_rows, ns, B, node_rows, nn, m, x_rows, nx, k),
which returns the k x m output scalars.

Run as a script it sends the shape, value and broadcast lists and two batches above the shard minimum through the host-pointer
entry in a process of its own bound to the device list given on the command line (a device may be listed twice, so one GPU still
crosses the shard split)."""
import os
import sys

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle"), os.path.join(_root, "tests")]

import fr_cases as fc  # noqa: E402

R = fc.R
G = 4                                                  # FR_LAGRANGE_G of csrc/fr29.hip.hpp (tests/test_fr_lagrange.py reads it from the harness)
SIZES_B = (1, 2, 3, 15, 16, 17, 63, 64, 65)
KM = (1, G - 1, G + 1, 63, 65, 1000)                   # numbers of outputs k m


def basis(S, node, x):
    num = den = 1
    for s in S:
        if (s - node) % R:
            num, den = num * (x - s) % R, den * (node - s) % R
    return num * pow(den, -1, R) % R


def basis_reference_loop(S, node, x):
    """ComputeLagrangeBasis(i, S, x): result *= (x - j) / (i - j) for every j in S with j != i, on field elements"""
    res = 1
    for s in S:
        if s % R != node % R:
            res = res * ((x - s) % R) * pow((node - s) % R, -1, R) % R
    return res


def expect(case):
    out = []
    for j in range(case["k"]):
        S = case["set"][j if len(case["set"]) > 1 else 0]
        N = S if case["nodes"] is None else case["nodes"][j if len(case["nodes"]) > 1 else 0]
        x = 0 if case["x"] is None else case["x"][j if len(case["x"]) > 1 else 0]
        out += [basis(S, t, x) for t in N]
    return out


def mk(label, sets, nodes, x, k=None):
    k = max(len(sets), len(nodes) if nodes else 1, len(x) if x else 1) if k is None else k
    return {"label": label, "set": sets, "nodes": nodes, "x": x, "k": k, "B": len(sets[0]), "m": len(nodes[0]) if nodes else len(sets[0])}


def rand_rows(tag, rows, n):
    v = fc.rand(tag, rows * n)
    return [v[i * n:(i + 1) * n] for i in range(rows)]


def size_cases():
    """every B of the list with the set as its own nodes (rows enough for several workgroups), and node lists of their own such that
    k m takes every value of KM; x = 0, one x, an x per row in turn"""
    out = []
    for i, B in enumerate(SIZES_B):
        k = 65 // B + 2
        x = (None, fc.rand("lx1-%d" % B, 1), fc.rand("lxk-%d" % B, k))[i % 3]
        out.append(mk("own-nodes-B%d" % B, rand_rows("ls-%d" % B, k, B), None, x))
    for i, km in enumerate(KM):
        for B in (SIZES_B[i], SIZES_B[i + 3]):
            k, m = (km // 8, 8) if km == 1000 else (1, km)
            sets = rand_rows("lks-%d-%d" % (km, B), k, B)
            nodes = rand_rows("lkn-%d-%d" % (km, B), k, m)
            for j in range(k):                          # a node inside the set, the others outside
                nodes[j][j % m] = sets[j][j % B]
            out.append(mk("km%d-B%d" % (km, B), sets, nodes, fc.rand("lkx-%d-%d" % (km, B), k)))
    return out


def geometry_cases():
    """the shapes at which the launch changes: the 256-element LDS form exactly full (16 rows x 16, 4 x 64) and just over it, rows
    per workgroup lowered to fit 1024 elements, a row over two workgroups (m > 256), a shared set in both LDS forms"""
    out = [mk("lds-full-16x16", rand_rows("g16", 40, 16), None, None),
           mk("lds-over-B17-m5", rand_rows("g17s", 70, 17), rand_rows("g17n", 70, 5), fc.rand("g17x", 70)),
           mk("rows-lowered-B65-m3", rand_rows("g65s", 70, 65), rand_rows("g65n", 70, 3), fc.rand("g65x", 1)),
           mk("two-workgroups-B300", rand_rows("g300", 3, 300), None, fc.rand("g300x", 3)),
           mk("shared-small-B17", [list(range(1, 18))], [list(range(17))], fc.rand("gsx", 130)),
           mk("shared-large-B300-m7", rand_rows("gl", 1, 300), rand_rows("gln", 1, 7), fc.rand("glx", 100))]
    return out


def value_cases():
    E = list(fc.EDGES)
    out = [mk("edges-own-nodes-x-edges", [E], None, E),                 # 0, r, 2r, 5r and 1, r + 1 are equal by value: all of them are skipped together
           mk("edges-as-nodes", [fc.rand("ve", 9)], [E], E),
           mk("edges-set-random-nodes", [E], [fc.rand("vn", 6)], None)]
    S = [1, R + 1, 0, 5 * R, 7, 9]                                      # equal only modulo r
    out.append(mk("equal-mod-r", [S], None, [3, 1, R, 12]))
    out.append(mk("equal-mod-r-node-unreduced", [[1, 2, 3]], [[R + 1, 2 * R + 2, 4 * R + 3, 4]], [5]))
    rep = [4, 9, 4, 11, 9, 4]                                           # one factor per occurrence
    out.append(mk("repeated", [rep], [[4, 9, 11, 5]], [2, 4, 0]))
    assert basis(rep, 11, 2) == (2 - 4) ** 3 * (2 - 9) ** 2 * pow((11 - 4) ** 3 * (11 - 9) ** 2, -1, R) % R
    out.append(mk("x-in-set", [[2, 5, 8]], None, [2, 5, 8, R + 5]))      # an indicator row
    z = rand_rows("vz", 4, 5)
    out.append(mk("x-omitted", z, None, None))
    out.append(mk("x-zero-rows", z, None, [0] * 4))
    out.append(mk("node-outside", [[3, 4, 5]], [[6, 0, 3]], [1, 2]))
    out.append(mk("all-nodes-skip", [[7, R + 7]], None, [3]))            # the empty product: 1
    return out


def broadcast_cases():
    """every combination of one set / a set per row, no nodes / one node row / a node row per row, no x / one x / an x per row, k = 5
    (all broadcast: five equal rows, which only the C entries can ask for)"""
    k, B, m = 5, 6, 4
    out = []
    for ns in (1, k):
        for nn in (0, 1, k):
            for nx in (0, 1, k):
                tag = "bc-%d-%d-%d" % (ns, nn, nx)
                out.append(mk(tag, rand_rows(tag + "s", ns, B), rand_rows(tag + "n", nn, m) if nn else None, fc.rand(tag + "x", nx) if nx else None, k=k))
    return out


def all_cases():
    return size_cases() + geometry_cases() + value_cases() + broadcast_cases()


def big_case():
    """B = m = 1024, two rows (the second one's x inside its set)"""
    sets = rand_rows("big", 2, 1024)
    return mk("B1024", sets, None, [fc.rand("bigx", 1)[0], sets[1][777]])


_EXPECT = {}


def expected(case):
    """computed once per process and shared between the tests"""
    if case["label"] not in _EXPECT:
        _EXPECT[case["label"]] = expect(case)
    return _EXPECT[case["label"]]


def flat(rows):
    return fc.rows([v for r in rows for v in r])


def run_cases(call, cases):
    """the labels of the cases whose output differs from Python's"""
    bad = []
    for c in cases:
        got = call(flat(c["set"]), len(c["set"]), c["B"], None if c["nodes"] is None else flat(c["nodes"]), len(c["nodes"]) if c["nodes"] else 0, c["m"],
                   None if c["x"] is None else fc.rows(c["x"]), len(c["x"]) if c["x"] else 0, c["k"])
        if fc.ints(got) != expected(c):
            bad.append(c["label"])
    return bad


def engine_call(eng, put=lambda a: a, back=lambda a: a):
    """the wrapper as run_cases' call; all-broadcast cases with k > 1 go to it row count 1 (it derives k from its arguments) and the
    one row is repeated for the comparison"""
    import numpy as np

    def call(s, ns, B, nd, nn, m, x, nx, k):
        got = back(eng.fr_lagrange_basis(put(s.reshape(-1)), B, None if nd is None else put(nd.reshape(-1)), None if nd is None else m, None if x is None else put(x.reshape(-1))))
        got = np.asarray(got).reshape(-1, m, 32)
        return np.repeat(got, k, axis=0) if got.shape[0] == 1 and k > 1 else got
    return call


def shard_case():
    """1100 rows x 16 own nodes: above twice the shard minimum (2^16 / 256 = 256 rows), with edge values and a short last workgroup"""
    c = mk("shard", rand_rows("sh", 1100, 16), None, None)
    for i, e in enumerate(fc.EDGES):
        c["set"][(i * 97) % 1100][i % 16] = e
    return c


if __name__ == "__main__":
    # python fr_lagrange_cases.py DEV [DEV ...]
    from gopairingbasedcryptography_amd import bn254 as engine
    engine.init([int(d) for d in sys.argv[1:]])
    shared = mk("shard-shared", [list(range(1, 18))], [list(range(17))], fc.rand("shx", 1000))       # 2^16 / 289 = 226 rows per shard at least
    failures = run_cases(engine_call(engine), geometry_cases() + value_cases() + broadcast_cases() + [shard_case(), shared])
    print("devices", engine.num_devices(), "failures", failures)
    sys.exit(1 if failures else 0)
