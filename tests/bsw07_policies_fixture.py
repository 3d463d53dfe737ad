"""Test helper: BSW07 with a policy per ciphertext, from the known secrets of tests/bsw07_fixture.py (alpha, beta, H(a) = [h_a] g) and the
user keys of tests/bsw07_keys_fixture.py, in the arrays bsw07.encrypt_batch_policies and bsw07.decrypt_batch_policies take: 12 items over
3 policies — the example tree, 2-of-3 and a single leaf — interleaved, 8 of them with attribute sets that satisfy their policy and 4
without, one of those holding some leaves of its policy all the same."""
import numpy as np

import bn254_py as o
import fr_cases as fc
import share_cases as shc
from bsw07_fixture import example_tree, sc
from bsw07_keys_fixture import GARBAGE, user_keys
from gopairingbasedcryptography_amd import bsw07

R = o.R
L, T = bsw07.Leaf, bsw07.Threshold
N = 12
POLICY_OF = [i % 3 for i in range(N)]
# per item, in item order: policy 0 is 2 of (11, 2 of (22, 33), 44, 1 of (55, 11)), policy 1 is 2 of (11, 22, 66), policy 2 is the leaf 44
SETS = [{11, 44}, {11, 22}, {44}, {22, 33, 55}, {22, 66}, {44, 11}, {22, 44}, {66}, {11}, {11}, set(), {44, 55}]
WANT_OK = [1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 0, 1]


def policies():
    return [example_tree(), T(2, L(11), L(22), L(66)), L(44)]


class Setup:
    """the public key, n messages, s and coefficients [n, Cmax] (random beyond an item's own C_t: they must not matter), the users' keys
    padded to Lmax with GARBAGE, all as host arrays"""

    def __init__(self, eng):
        self.trees = policies()
        self.plan = bsw07.forest_plan(self.trees)
        plans, self.attributes, self.index = self.plan
        self.L = [len(a) for _, a in plans]
        self.C = [shc.n_coeffs(t) for t in self.trees]
        self.Lmax, self.Cmax = max(self.L), max(self.C)
        g1, g2 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8), np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
        alpha, beta = sc("alpha"), sc("beta")
        e = eng.pair_batch(g1, g2)
        self.e_alpha = np.asarray(eng.gt_exp(e, [alpha])[0])
        self.h = np.asarray(eng.g1_scalar_mul(g1, [beta])[0])
        self.h1 = {a: np.asarray(eng.g1_scalar_mul(g1, [sc("h", a)])[0]) for a in self.attributes}
        self.msgs = np.stack([np.asarray(eng.gt_exp(e, [sc("policies-msg", i)])[0]) for i in range(N)])
        self.s = fc.rows([sc("policies-s", i) for i in range(N)])
        self.coeffs = fc.rows([sc("policies-q", i) for i in range(N * self.Cmax)]).reshape(N, self.Cmax, 32)
        self.policy_of = np.array(POLICY_OF, dtype=np.uint32)
        self.held = bsw07.leaf_mask_policies(self.plan, POLICY_OF, SETS)
        self.D = np.zeros((N, 128), dtype=np.uint8)
        self.dj, self.djp = np.full((N, self.Lmax, 128), GARBAGE, dtype=np.uint8), np.full((N, self.Lmax, 128), GARBAGE, dtype=np.uint8)
        for t, tree in enumerate(self.trees):
            items = [i for i in range(N) if POLICY_OF[i] == t]
            D, dj, djp, _, _ = user_keys(eng, tree, [SETS[i] for i in items])
            self.D[items], self.dj[items, :self.L[t]], self.djp[items, :self.L[t]] = D, dj, djp

    def items(self, t):
        return [i for i in range(N) if POLICY_OF[i] == t]

    def per_policy(self, eng, t, tables=False):
        """bsw07.encrypt_batch under policy t alone on that policy's items: the same s, the first C_t columns of their coefficients"""
        rows = self.items(t)
        q = np.ascontiguousarray(self.coeffs[rows, :self.C[t]]) if self.C[t] else None
        return bsw07.encrypt_batch(eng, self.trees[t], self.h, self.e_alpha, self.h1, self.msgs[rows], self.s[rows], q, tables=tables)


def same_as_per_policy(setup, got, per_policy, back=np.asarray):
    """got = (c_tilde, c, cy, cy_prime) of encrypt_batch_policies against per_policy[t] = encrypt_batch's of policy t: equal byte for byte
    in the first L_t columns, all zero in the padded ones"""
    c_tilde, c, cy, cyp = [back(g) for g in got]
    assert c_tilde.shape == (N, 384) and c.shape == (N, 64) and cy.shape == cyp.shape == (N, setup.Lmax, 64)
    for t, want in enumerate(per_policy):
        rows, Lt = setup.items(t), setup.L[t]
        w = [np.asarray(a) for a in want]                                                 # per_policy ran on host arrays
        assert c_tilde[rows].tobytes() == w[0].tobytes() and c[rows].tobytes() == w[1].tobytes(), t
        assert cy[rows, :Lt].tobytes() == w[2].tobytes() and cyp[rows, :Lt].tobytes() == w[3].tobytes(), t
        assert w[2].any() and w[3].any() and not cy[rows, Lt:].any() and not cyp[rows, Lt:].any(), t
    return True
