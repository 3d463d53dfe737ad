"""Test helper: BSW07 keys of many users under one policy, from the known secrets of tests/bsw07_fixture.py (alpha, beta, H(a) = [h_a] g),
in the arrays bsw07.decrypt_batch_keys takes (the stand-in engine of its plan test is tests/standin_engine.py).

KeyGenerate (cpabe/bsw07/bsw07_cpabe.go:97-130) for user u with attributes A_u: D = g2^((alpha + r_u) / beta) and per attribute a
Dj = g2^r_u H2(a)^rj, Dj' = g2^rj.  With H2(a) = [h_a] g2 every component is a multiple of the generator by a known scalar, so the keys
of all users are three calls of the engine's g2_scalar_mul_base."""
import numpy as np

import bn254_py as o
import fr_cases as fc
from bsw07_fixture import leaves, sc

R = o.R
GARBAGE = 0xEE                       # what the rows of leaves a key does not hold are filled with: no point, and it must not matter


def user_keys(eng, tree, attr_sets):
    """(D [n, 128], dj [n, L, 128], dj_prime [n, L, 128], per user {attribute: Dj}, {attribute: Dj'}) with the leaves in leaf-id order"""
    alpha, beta = sc("alpha"), sc("beta")
    attrs = [l.attribute for l in leaves(tree)]
    n, L = len(attr_sets), len(attrs)
    r = [sc("r-user", u) for u in range(n)]
    D = np.asarray(eng.g2_scalar_mul_base(fc.rows([(alpha + ru) * pow(beta, -1, R) % R for ru in r]).reshape(-1))).reshape(n, 128)
    slots = [(u, y) for u in range(n) for y in range(L) if attrs[y] in attr_sets[u]]
    rj = {(u, a): sc("rj-user-%d" % u, a) for u in range(n) for a in attr_sets[u]}
    kj = [(r[u] + sc("h", attrs[y]) * rj[u, attrs[y]]) % R for u, y in slots]
    kjp = [rj[u, attrs[y]] for u, y in slots]
    dj, djp = np.full((n, L, 128), GARBAGE, dtype=np.uint8), np.full((n, L, 128), GARBAGE, dtype=np.uint8)
    by_attr, by_attr_p = [{} for _ in range(n)], [{} for _ in range(n)]
    if slots:
        pj = np.asarray(eng.g2_scalar_mul_base(fc.rows(kj).reshape(-1))).reshape(-1, 128)
        pjp = np.asarray(eng.g2_scalar_mul_base(fc.rows(kjp).reshape(-1))).reshape(-1, 128)
        for i, (u, y) in enumerate(slots):
            dj[u, y], djp[u, y] = pj[i], pjp[i]
            by_attr[u][attrs[y]], by_attr_p[u][attrs[y]] = pj[i], pjp[i]
    return D, dj, djp, by_attr, by_attr_p


def ciphertext_arrays(inst, picks):
    """(c_tilde, c, cy, cy_prime) of the fixture's ciphertexts picks[t], columns in leaf-id order"""
    ids = [l.leaf_id for l in leaves(inst.tree)]
    cts = [inst.cts[t] for t in picks]
    return (np.stack([np.asarray(ct["c_tilde"]) for ct in cts]), np.stack([np.asarray(ct["c"]) for ct in cts]),
            np.stack([np.stack([np.asarray(ct["cy"][i]) for i in ids]) for ct in cts]), np.stack([np.stack([np.asarray(ct["cy_prime"][i]) for i in ids]) for ct in cts]))
