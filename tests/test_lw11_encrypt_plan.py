"""LW11 decentralised ABE Encrypt through the host planner (gopairingbasedcryptography_amd/lw11.py: encrypt_batch) on the oracle
stand-in engine (tests/standin_engine.py; the same flow runs on the GPU engine in test_lsss_encrypt_gpu.py): fed the fixture's own
secrets it returns the fixture's ciphertext bytes, and the existing decrypt_batch / decrypt_batch_msm recover the messages — for the
AND / OR policy and for 3 of 5 as Shamir rows, whose weights are neither 0 nor 1."""
import numpy as np
import pytest

import bn254_py as o
import gmsm_cases as gc
from lw11_fixture import Instance, and_or_policy, sc as fsc, threshold_policy
from standin_engine import StandInEngine, TensorEngine, same_on_tensors, tensors
from sw05_fixture import kbytes
from gopairingbasedcryptography_amd import lw11

G1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
G2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
N = 3


def fixture_inputs(inst, tag=""):
    """what Instance drew, by its sc(tag, i) names: the authorities' public keys and the per-ciphertext randomness"""
    eng, C, n = inst.eng, len(inst.matrix[0]), inst.n
    attrs = sorted(set(inst.rho))
    e = np.asarray(inst.e).reshape(384)
    ea = np.asarray(eng.gt_exp(np.tile(e, (len(attrs), 1)), [fsc(tag + "alpha", a) for a in attrs])).reshape(-1, 384)
    gy = np.asarray(eng.g2_scalar_mul(G2, [fsc(tag + "y", a) for a in attrs])).reshape(-1, 128)
    return dict(e=e, egg_alpha={a: ea[i] for i, a in enumerate(attrs)}, g2_y={a: gy[i] for i, a in enumerate(attrs)},
                s=[fsc(tag + "v0", t) for t in range(n)], v=[[fsc(tag + "v%d" % j, t) for j in range(1, C)] for t in range(n)],
                w=[[fsc(tag + "w%d" % j, t) for j in range(1, C)] for t in range(n)], r=[[fsc(tag + "r%d" % x, t) for x in range(inst.R)] for t in range(n)])


def encrypt(eng, inst, f, msgs=None, **kw):
    a = dict(f, **kw)
    return lw11.encrypt_batch(eng, a["e"], a["egg_alpha"], a["g2_y"], a.get("matrix", inst.matrix), a.get("rho", inst.rho), np.asarray(inst.msgs) if msgs is None else msgs,
                              a["s"], a["v"], a["w"], a["r"], table=a.get("table"))


POLICIES = {"and-or": (and_or_policy, [11, 22, 44, 99]), "3of5": (lambda: threshold_policy(3, 5), [200, 202, 203])}


@pytest.fixture(scope="module", params=list(POLICIES))
def setup(oracle, request):
    eng = StandInEngine(oracle)
    make, held = POLICIES[request.param]
    m, rho = make()
    inst = Instance(eng, m, rho, held, n_ct=N)
    return eng, inst, fixture_inputs(inst)


def test_encrypt_batch_returns_the_fixture_ciphertexts(setup):
    eng, inst, f = setup
    got = encrypt(eng, inst, f)
    Rr = inst.R
    for g, w, shape in zip(got, (inst.c0, inst.c1, inst.c2, inst.c3), ((N, 384), (N, Rr, 384), (N, Rr, 128), (N, Rr, 128))):
        assert g.shape == shape and np.asarray(g).tobytes() == np.asarray(w).tobytes()
    assert eng.tables[-1].closed and eng.tables[-1].g2 and eng.tables[-1].nbase == 1 + len(set(inst.rho))
    table = lw11.encrypt_table(eng, f["g2_y"])
    again = encrypt(eng, inst, f, s=kbytes(f["s"]).reshape(-1, 32), v=kbytes([x for r in f["v"] for x in r]).reshape(N, -1, 32), w=kbytes([x for r in f["w"] for x in r]).reshape(N, -1, 32),
                    r=kbytes([x for r in f["r"] for x in r]).reshape(N, -1, 32), table=table)
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(again, got)) and not table.closed and table.calls == 1


def test_decrypt_of_the_encrypted_batch_returns_the_messages(setup):
    eng, inst, f = setup
    c0, c1, c2, c3 = encrypt(eng, inst, f)
    rows, w = lw11.reconstruction_weights(inst.matrix, inst.rho, inst.user_attrs)
    folded = lw11.fold_key(eng, rows, w, inst.h_gid, inst.k_by_row)
    out = lw11.decrypt_batch(eng, folded, c0, c1, c2, c3)
    assert np.asarray(out).tobytes() == np.asarray(inst.msgs).tobytes()
    eng.g2_multi_scalar_mul = lambda bases, scalars, seg_off: gc.expect(eng.o, True, np.asarray(bases, dtype=np.uint8).reshape(-1, 128), [int(k) for k in scalars], [int(v) for v in seg_off],
                                                                       len(scalars) != np.asarray(bases).size // 128)
    out2 = lw11.decrypt_batch_msm(eng, folded, inst.h_gid, c0, c1, c2, c3)
    assert np.asarray(out2).tobytes() == np.asarray(inst.msgs).tobytes()


def test_encrypt_on_tensors_is_encrypt_on_arrays(setup):
    eng, inst, f = setup
    want = encrypt(eng, inst, f)
    flat = lambda rows: kbytes([x for r in rows for x in r]).reshape(N, -1, 32)
    tm, ts, tv, tw, tr = tensors(np.asarray(inst.msgs), kbytes(f["s"]).reshape(-1, 32), flat(f["v"]), flat(f["w"]), flat(f["r"]))
    got = encrypt(TensorEngine(eng), inst, f, msgs=tm, s=ts, v=tv, w=tw, r=tr)
    assert all(same_on_tensors(g, np.asarray(w)) for g, w in zip(got, want))


def test_attributes_outside_the_universe_and_argument_errors(setup):
    eng, inst, f = setup
    gone = inst.rho[1]
    n_tables = len(eng.tables)
    with pytest.raises(ValueError, match="is not in the universe"):
        encrypt(eng, inst, f, g2_y={a: p for a, p in f["g2_y"].items() if a != gone})
    with pytest.raises(ValueError, match="is not in the universe"):
        encrypt(eng, inst, f, egg_alpha={a: p for a, p in f["egg_alpha"].items() if a != gone})
    assert len(eng.tables) == n_tables                                                   # refused before the engine is touched
    small = lw11.encrypt_table(eng, {a: p for a, p in f["g2_y"].items() if a != gone})
    for bad in (lambda: encrypt(eng, inst, f, s=f["s"][:2]), lambda: encrypt(eng, inst, f, v=[r[:-1] for r in f["v"]]), lambda: encrypt(eng, inst, f, w=[r[:-1] for r in f["w"]]),
                lambda: encrypt(eng, inst, f, r=[r[:-1] for r in f["r"]]), lambda: encrypt(eng, inst, f, rho=inst.rho[:-1]), lambda: encrypt(eng, inst, f, matrix=[]),
                lambda: encrypt(eng, inst, f, msgs=np.asarray(inst.msgs).reshape(-1)[:-1]), lambda: encrypt(eng, inst, f, table=small)):
        with pytest.raises(ValueError):
            bad()
