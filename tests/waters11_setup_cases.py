"""Cases and expectations of the Waters11 SetUp tests (tests/test_waters11_setup_plan.py on the stand-in engine,
tests/test_waters11_setup_gpu.py on the GPU): the secrets, the oracle's g1a = [a] g1, g1_alpha = [alpha] g1, e_alpha = e(g1, g2)^alpha and
h_u = [tau_u] g1 on them — one generator multiplication each, one pairing and one power, nothing from the planner — the check of a
(pp, msk) pair against them, and the round trip on a universe of 5, a 3-row policy and 2 users."""
import numpy as np

import bn254_py as o
from sw05_fixture import kbytes
from gopairingbasedcryptography_amd import waters11

R = o.R
G1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
G2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
SEED = bytes(range(32))
UNIVERSE = [40, 7, 19, 3, 25]                                                  # unsorted on purpose: tau[i] belongs to sorted(UNIVERSE)[i]
POLICY = ([[1, 1, 0], [0, R - 1, 1], [0, 0, R - 1]], [3, 19, 40])              # 3 and 19 and 40
USERS = [[40, 3, 19, 7], [3, 19, 25]]


def sc(tag, i=0):
    return o.bench_scalar("waters11-setup-" + tag, i)


ALPHA, A, TAU = sc("alpha"), sc("a"), [sc("tau", i) for i in range(len(UNIVERSE))]


def expected(oracle, universe, tau):
    """(g1a, g1_alpha, e_alpha, h) from the secrets: one generator multiplication each, one pairing and one power"""
    pts = np.asarray(oracle.g1_scalar_mul(G1, kbytes([A, ALPHA] + list(tau)))).reshape(-1, 64)
    e_alpha = np.asarray(oracle.gt_exp(oracle.pair_batch(G1, G2), kbytes([ALPHA]))).reshape(384)
    return pts[0], pts[1], e_alpha, {u: pts[2 + i] for i, u in enumerate(sorted(universe))}


def check(pp, msk, want, back=np.asarray):
    g1a, g1_alpha, e_alpha, h = want
    assert sorted(pp) == ["e_alpha", "g1a", "h"] and sorted(msk) == ["g1_alpha"]
    assert all(isinstance(pp[k], np.ndarray) for k in ("g1a", "e_alpha")) and pp["g1a"].shape == (64,) and pp["e_alpha"].shape == (384,)
    assert pp["g1a"].tobytes() == g1a.tobytes() and pp["e_alpha"].tobytes() == e_alpha.tobytes()
    assert tuple(msk["g1_alpha"].shape) == (64,) and back(msk["g1_alpha"]).tobytes() == g1_alpha.tobytes()
    assert sorted(pp["h"]) == sorted(h) and all(isinstance(p, np.ndarray) and p.shape == (64,) and p.tobytes() == h[u].tobytes() for u, p in pp["h"].items())


def round_trip(eng, oracle, put=lambda a: a, back=np.asarray):
    """setup -> keygen_batch -> encrypt_batch -> decrypt_batch on a universe of 5, a 3-row policy and 2 users"""
    pp, msk = waters11.setup(eng, UNIVERSE, put(kbytes([ALPHA])), put(kbytes([A])), put(kbytes(TAU)))
    K, L, kx, attrs = waters11.keygen_batch(eng, msk["g1_alpha"], pp["g1a"], pp["h"], USERS, put(kbytes([sc("t", j) for j in range(2)])))
    e = np.asarray(oracle.pair_batch(G1, G2)).reshape(1, 384)
    msgs = np.asarray(oracle.gt_exp(np.tile(e, (2, 1)), kbytes([sc("msg", i) for i in range(2)]))).reshape(2, 384)
    s, v, r = kbytes([sc("s", i) for i in range(2)]), kbytes([sc("v", i) for i in range(4)]), kbytes([sc("r", i) for i in range(6)])
    ct = waters11.encrypt_batch(eng, pp["g1a"], pp["e_alpha"], pp["h"], [POLICY, POLICY], put(msgs), put(s), put(v.reshape(2, 2, 32)), put(r.reshape(2, 3, 32)))
    for j, satisfied in enumerate((True, False)):
        key = (back(K)[j], back(L)[j], {int(u): back(kx)[j, i] for i, u in enumerate(attrs[j]) if u >= 0})
        out, ok = waters11.decrypt_batch(eng, key, [POLICY, POLICY], *ct)
        assert back(ok).tolist() == [int(satisfied)] * 2
        assert back(out).tobytes() == (msgs.tobytes() if satisfied else bytes(2 * 384)), j
