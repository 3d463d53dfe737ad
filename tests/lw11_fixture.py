"""Test helper: an LW11 decentralised ABE instance (dabe/lw11_dabe.go:63-174) built from known secrets with any engine that has the
bn254 module's function names — AuthoritySetup, KeyGenerate and Encrypt restated on exponents: every group element is ONE
multiplication of a generator by the exponent the reference's Exp / Mul / Add sequence arrives at (canonical bytes, so the same
element), through the engine's entries OTHER than the ones under test (pair_batch, gt_exp, g1 / g2 scalar multiplication of a
shared base).  H(GID) is a stand-in point [h] g1 (hash to curve is not what is tested here).  Encrypt shares over every ROW of the
matrix, as the scheme does (the reference's loop runs to the column count, lw11_dabe.go:111,139: the same thing for its square
test matrices).

numpy arrays by default; with `dev` a torch device everything per ciphertext is made and kept in HBM (the instances at size)."""
import numpy as np

import bn254_py as o


def sc(tag, i=0):
    return o.bench_scalar("lw11-" + tag, i)


def kbytes(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8)


# ---- policies: (matrix, rho)
def and_or_policy():
    """(A and B) or (C and D) as a Lewko-Waters matrix: 4 rows, 3 columns, attributes 11, 22, 33, 44; every solution has weights 1"""
    return [[1, 1, 0], [0, -1, 0], [1, 0, 1], [0, 0, -1]], [11, 22, 33, 44]


def and_chain_policy(rows):
    """A_1 and ... and A_rows: row 0 = (1, 1, 0, ...), row i = (0, ..., -1 at i, 1 at i + 1, ...), the last (0, ..., -1); all weights 1"""
    m = [[0] * rows for _ in range(rows)]
    for i in range(rows):
        m[i][i] = 1 if i == 0 else -1
        if i + 1 < rows:
            m[i][i + 1] = 1
    if rows == 1:
        m = [[1]]
    return m, [100 + i for i in range(rows)]


def threshold_policy(t, rows):
    """t of `rows` attributes as Shamir rows (1, x, x^2, ..., x^(t-1)), x = 1 .. rows: the weights are Lagrange coefficients, neither 0 nor 1"""
    return [[pow(x, j, o.R) for j in range(t)] for x in range(1, rows + 1)], [200 + i for i in range(rows)]


class Instance:
    def __init__(self, eng, matrix, rho, user_attrs, n_ct, dev=None, tag=""):
        self.eng, self.matrix, self.rho, self.user_attrs, self.n, self.dev = eng, matrix, rho, set(user_attrs), n_ct, dev
        R, C = len(matrix), len(matrix[0])
        self.R = R
        if dev is not None:
            import torch
            put = lambda a: torch.from_numpy(np.array(a, dtype=np.uint8, copy=True)).to(dev)
        else:
            put = lambda a: np.array(a, dtype=np.uint8, copy=True)
        g1, g2 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8), np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
        self.e = np.asarray(eng.pair_batch(g1, g2)).reshape(1, 384)                       # GlobalSetup
        alpha = {a: sc(tag + "alpha", a) for a in set(rho)}                                # AuthoritySetup: SK = {alpha_i, y_i}
        y = {a: sc(tag + "y", a) for a in set(rho)}
        h = sc(tag + "gid")
        self.h_gid = np.asarray(eng.g1_scalar_mul(g1, [h])).reshape(64)                   # H(GID) = [h] g1
        held = sorted(a for a in set(rho) if a in self.user_attrs)
        K = np.asarray(eng.g1_scalar_mul(g1, [(alpha[a] + h * y[a]) % o.R for a in held])).reshape(-1, 64) if held else np.zeros((0, 64), np.uint8)
        k_by_attr = {a: K[i] for i, a in enumerate(held)}                                  # KeyGenerate: K_i = g1^alpha_i H(GID)^y_i
        self.k_by_row = {x: k_by_attr[rho[x]] for x in range(R) if rho[x] in k_by_attr}
        # Encrypt, n_ct times: v = (s, v_2, ...), w = (0, w_2, ...), lambda_x = M_x . v, omega_x = M_x . w, r_x random
        M = np.array([[int(v) % o.R for v in row] for row in matrix], dtype=object)
        V = np.array([[sc(tag + "v%d" % j, t) for t in range(n_ct)] for j in range(C)], dtype=object)      # row 0 = the secrets s
        W = np.array([[0 if j == 0 else sc(tag + "w%d" % j, t) for t in range(n_ct)] for j in range(C)], dtype=object)
        lam, om = M.dot(V) % o.R, M.dot(W) % o.R                                           # [R, n]
        rx = np.array([[sc(tag + "r%d" % x, t) for t in range(n_ct)] for x in range(R)], dtype=object)
        al = np.array([alpha[a] for a in rho], dtype=object).reshape(R, 1)
        yy = np.array([y[a] for a in rho], dtype=object).reshape(R, 1)
        msg = [sc(tag + "msg", t) for t in range(n_ct)]
        flat = lambda a: [int(v) for v in a.T.reshape(-1)]                                 # ciphertext-major: index t * R + x
        gexp = lambda ks: eng.gt_exp(put(np.tile(self.e, (len(ks), 1))), put(kbytes(ks)))
        g2mul = lambda ks: eng.g2_scalar_mul(put(g2), put(kbytes(ks)))
        self.msgs = gexp(msg)                                                              # M_t = e(g1, g2)^msg_t
        self.c0 = gexp([(m + s) % o.R for m, s in zip(msg, V[0])])                         # M e(g1, g2)^s
        self.c1 = gexp(flat((lam + al * rx) % o.R))                                        # e(g1, g2)^lambda_x e(g1, g2)^(alpha_rho(x) r_x)
        self.c2 = g2mul(flat(rx))                                                          # g2^r_x
        self.c3 = g2mul(flat((yy * rx + om) % o.R))                                        # g2^(y_rho(x) r_x) g2^omega_x

    def ct(self, t):
        """ciphertext t on the host: c0 [384], c1 [R, 384], c2, c3 [R, 128]"""
        host = lambda a: (a.cpu().numpy() if self.dev is not None else np.asarray(a))
        R = self.R
        return (host(self.c0.reshape(-1, 384)[t]), host(self.c1.reshape(-1, 384)[t * R:(t + 1) * R]),
                host(self.c2.reshape(-1, 128)[t * R:(t + 1) * R]), host(self.c3.reshape(-1, 128)[t * R:(t + 1) * R]))

    def row_by_row_decrypt(self, oracle, t, rows, weights, running):
        """Decrypt of lw11_dabe.go:176-203 with oracle calls, one pairing at a time, Mul / Mul / Div / Exp per row.
        running = True is the loop as written: the RUNNING product is raised at every row, and the weight is taken from the
        compacted slice at the matrix row number (wSlice[x]); running = False raises each row's own term to its weight and
        multiplies (the scheme).  They agree when all weights are 1."""
        c0, c1, c2, c3 = self.ct(t)
        one = np.frombuffer(o.gt_to_bytes(o.F12_ONE), dtype=np.uint8)
        den = one
        for pos, x in enumerate(rows):
            cur = den if running else one
            cur = oracle.gt_mul(cur, c1[x])[0]
            cur = oracle.gt_mul(cur, oracle.pair_batch(self.h_gid, c3[x])[0])[0]
            cur = oracle.gt_div(cur, oracle.pair_batch(self.k_by_row[x], c2[x])[0])[0]
            w = weights[x] if running else weights[pos]
            cur = oracle.gt_exp(cur, kbytes([w]))[0]
            den = cur if running else oracle.gt_mul(den, cur)[0]
        return oracle.gt_div(c0, den)[0]
