"""bibe/gwww25_bibe/gwww25_bibe.go (:82-256) and gwww25_bibe_utils.go (:9-50) transcribed line by line onto the C oracle and Python integers
modulo r, one call at a time: what tests/test_gwww25_plan.py (stand-in engine) and tests/test_gwww25_gpu.py (the device) hold the planner
gopairingbasedcryptography_amd/gwww25.py against.  Shares nothing with the planner or the kernels."""
import numpy as np

import bn254_py as o
from sw05_fixture import kbytes

R = o.R
G1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
G2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)


def sc(tag, i=0):
    return o.bench_scalar("gwww25-" + tag, i) % R


def row(x):
    return np.asarray(x, dtype=np.uint8).reshape(-1)


class Ref:
    """gwww25_bibe.go on the oracle, one call at a time, every line the reference's"""

    def __init__(self, orc, B):
        self.orc = orc
        self.tau, self.w, self.v, self.h, self.alpha = (sc(name) for name in ("tau", "w", "v", "h", "alpha"))
        mul1 = lambda k: row(orc.g1_scalar_mul(G1, kbytes([k])))
        self.g1_tau, self.g1_w = mul1(self.tau), mul1(self.w)                                  # :93-94
        self.g1_wtau = mul1(self.tau * self.w % R)                                             # :95-96
        self.g1_v, self.g1_h = mul1(self.v), mul1(self.h)                                      # :97-98
        e = orc.pair_batch(G1, G2)[0]                                                          # :101
        self.gt_alpha = row(orc.gt_exp(e, kbytes([self.alpha])))                               # :105
        power, self.powers = self.tau, []                                                      # :107-112
        for _ in range(B):
            self.powers.append(row(orc.g2_scalar_mul(G2, kbytes([power]))))
            power = power * self.tau % R

    def encrypt(self, m, ident, tg, s):
        orc = self.orc
        ct1 = row(orc.g1_scalar_mul(G1, kbytes([s])))                                          # :137
        swtau1 = orc.g1_scalar_mul(self.g1_wtau, kbytes([s]))[0]                               # :140
        sid = s * ident % R                                                                    # :141
        sidw1 = orc.g1_scalar_mul(self.g1_w, kbytes([sid]))[0]                                 # :142
        neg = np.frombuffer(o.g1_to_bytes(o.g1_neg(o.g1_from_bytes(sidw1.tobytes()))), dtype=np.uint8)
        ct2 = row(orc.g1_sum(np.stack([swtau1, neg])))                                          # :143 Sub
        tgh1 = orc.g1_scalar_mul(self.g1_h, kbytes([tg]))[0]                                   # :146
        v1_add = row(orc.g1_sum(np.stack([self.g1_v, tgh1])))                                  # :147
        ct3 = row(orc.g1_scalar_mul(v1_add, kbytes([s])))                                      # :148
        ct4 = row(orc.gt_mul(orc.gt_exp(self.gt_alpha, kbytes([s]))[0], m))                    # :151-152
        return ct1, ct2, ct3, ct4

    def coeffs(self, identities):                                                              # computePolynomialCoeffs, utils :9-38
        c = [1]
        for ident in identities:
            new = [0] * (len(c) + 1)
            for i in range(len(c)):
                new[i] = (new[i] + (-(ident * c[i])) % R) % R
                new[i + 1] = (new[i + 1] + c[i]) % R
            c = new
        return c

    def g2_poly_tau(self, coef):                                                               # computeG2PolynomialTau, utils :40-50
        result = row(self.orc.g2_scalar_mul(G2, kbytes([coef[0]])))
        for i in range(1, len(coef)):
            term = row(self.orc.g2_scalar_mul(self.powers[i - 1], kbytes([coef[i]])))
            result = row(self.orc.g2_sum(np.stack([result, term])))
        return result

    def digest(self, identities):                                                              # :162-176
        if len(identities) == 0:
            raise ValueError("identities is empty")
        if len(identities) > len(self.powers):
            raise ValueError("too many identities for batch size")
        return self.g2_poly_tau(self.coeffs(identities))

    def compute_key(self, d, tg, r, y):                                                        # :178-209
        u1 = row(self.orc.g2_scalar_mul(G2, kbytes([r])))
        yw = y * self.w % R
        ywd2 = row(self.orc.g2_scalar_mul(d, kbytes([yw])))
        temp = self.h * tg % R
        temp = (self.v + temp) % R
        temp = r * temp % R
        temp = (self.alpha + temp) % R
        g2_temp = row(self.orc.g2_scalar_mul(G2, kbytes([temp])))
        return y, u1, row(self.orc.g2_sum(np.stack([ywd2, g2_temp])))

    def decrypt(self, sk, identities, ident, ct):                                              # :211-256
        y, u1, u2 = sk
        without = [x for x in identities if x % R != ident % R]
        if len(without) != len(identities) - 1:
            raise ValueError("identity not found in identity list")
        pi = self.g2_poly_tau(self.coeffs(without))
        pair_a = self.orc.pair_batch(ct[0], u2)[0]
        yct2 = row(self.orc.g1_scalar_mul(ct[1], kbytes([y])))
        pair_b = self.orc.pair_batch(yct2, pi)[0]
        pair_c = self.orc.pair_batch(ct[2], u1)[0]
        temp1 = self.orc.gt_div(pair_a, pair_b)[0]
        temp2 = self.orc.gt_div(temp1, pair_c)[0]
        return row(self.orc.gt_div(ct[3], temp2))
