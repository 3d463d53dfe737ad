"""Waters11 CP-ABE Encrypt and KeyGenerate through the host planner (gopairingbasedcryptography_amd/waters11.py: encrypt_batch,
keygen_batch) on the oracle stand-in engine (tests/standin_engine.py; the same flow runs on the GPU engine in
test_lsss_encrypt_gpu.py): fed the fixture's own secrets it returns the fixture's ciphertext bytes on every real row and the point at
infinity on every padding row, the existing decrypt_batch recovers the messages (and reports the policy the key does not satisfy),
and keygen_batch returns the fixture's key construction."""
import numpy as np
import pytest

import bn254_py as o
from standin_engine import StandInEngine, TensorEngine, same_on_tensors, tensors
from sw05_fixture import kbytes
from waters11_fixture import Instance, sc as fsc, small_policies
from gopairingbasedcryptography_amd import waters11

R = o.R
G1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
G2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)


def fixture_inputs(inst, tag=""):
    """what Instance drew, by its sc(tag, i) names: the public key, the universe's h_u and the per-ciphertext randomness, v padded with
    zeros to the widest policy (a padded column of the matrix is zero) and r for all R rows"""
    eng = inst.eng
    a, alpha = fsc(tag + "a"), fsc(tag + "alpha")
    universe = sorted(set(inst.key_attrs) | {u for _, rho in inst.policies for u in rho})
    g1a = np.asarray(eng.g1_scalar_mul(G1, [a])).reshape(64)
    g1_alpha = np.asarray(eng.g1_scalar_mul(G1, [alpha])).reshape(64)
    e_alpha = np.asarray(eng.gt_exp(np.asarray(eng.pair_batch(G1, G2)).reshape(384), [alpha])).reshape(384)
    hs = np.asarray(eng.g1_scalar_mul(G1, [fsc(tag + "tau", u) for u in universe])).reshape(-1, 64)
    h = {u: hs[i] for i, u in enumerate(universe)}
    C = max(len(m[0]) for m, _ in inst.policies)
    s = [fsc(tag + "s", j) for j in range(inst.n)]
    v = [[fsc(tag + "v%d" % c, j) if c < len(m[0]) else 0 for c in range(1, C)] for j, (m, _) in enumerate(inst.policies)]
    r = [[fsc(tag + "r%d" % x, j) for x in range(inst.R)] for j in range(inst.n)]
    return dict(g1a=g1a, g1_alpha=g1_alpha, e_alpha=e_alpha, h=h, s=s, v=v, r=r)


def check_ciphertexts(inst, got, back=np.asarray):
    c, c_prime, cx, dx = [back(g) for g in got]
    n, Rr = inst.n, inst.R
    assert c.shape == (n, 384) and c_prime.shape == (n, 128) and cx.shape == (n, Rr, 64) and dx.shape == (n, Rr, 128)
    assert c.tobytes() == np.asarray(inst.c).tobytes() and c_prime.tobytes() == np.asarray(inst.c_prime).tobytes()
    assert dx.tobytes() == np.asarray(inst.dx).tobytes()
    want = np.asarray(inst.cx).reshape(n, Rr, 64)
    for j, (m, _) in enumerate(inst.policies):
        assert cx[j, :len(m)].tobytes() == want[j, :len(m)].tobytes(), j
        assert not cx[j, len(m):].any(), j                                           # padding rows: the infinity encoding
    assert any(len(m) < Rr for m, _ in inst.policies)


@pytest.fixture(scope="module")
def setup(oracle):
    eng = StandInEngine(oracle)
    policies, key_attrs = small_policies()
    inst = Instance(eng, key_attrs, policies)
    return eng, inst, fixture_inputs(inst)


def test_encrypt_batch_returns_the_fixture_ciphertexts(setup):
    eng, inst, f = setup
    msgs = np.asarray(inst.msgs)
    got = waters11.encrypt_batch(eng, f["g1a"], f["e_alpha"], f["h"], inst.policies, msgs, f["s"], f["v"], f["r"])
    check_ciphertexts(inst, got)
    assert eng.tables[-1].closed and eng.tables[-1].nbase == 1 + len(f["h"])         # the table built here is closed here
    # the padded block and scalars as bytes are the same call; a table built once serves it and stays open
    pad = waters11.pad_policies(inst.policies)
    table = waters11.encrypt_table(eng, f["g1a"], f["h"])
    again = waters11.encrypt_batch(eng, f["g1a"], f["e_alpha"], f["h"], pad, msgs, kbytes(f["s"]).reshape(-1, 32), kbytes([x for r in f["v"] for x in r]).reshape(inst.n, -1, 32),
                                   kbytes([x for r in f["r"] for x in r]).reshape(inst.n, -1, 32), table=table)
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(again, got)) and not table.closed and table.calls == 1


def test_decrypt_of_the_encrypted_batch_returns_the_messages(setup):
    eng, inst, f = setup
    msgs = np.asarray(inst.msgs).reshape(-1, 384)
    c, c_prime, cx, dx = waters11.encrypt_batch(eng, f["g1a"], f["e_alpha"], f["h"], inst.policies, msgs, f["s"], f["v"], f["r"])
    out, ok = waters11.decrypt_batch(eng, inst.key, inst.policies, c, c_prime, cx, dx)
    sat = inst.satisfied()
    assert sat == [True, True, True, False] and ok.tolist() == [1, 1, 1, 0]
    for j in range(inst.n):
        assert np.asarray(out)[j].tobytes() == (msgs[j].tobytes() if sat[j] else bytes(384)), j


def test_encrypt_on_tensors_is_encrypt_on_arrays(setup):
    eng, inst, f = setup
    msgs = np.asarray(inst.msgs)
    want = waters11.encrypt_batch(eng, f["g1a"], f["e_alpha"], f["h"], inst.policies, msgs, f["s"], f["v"], f["r"])
    tm, ts, tv, tr = tensors(msgs, kbytes(f["s"]).reshape(-1, 32), kbytes([x for r in f["v"] for x in r]).reshape(inst.n, -1, 32), kbytes([x for r in f["r"] for x in r]).reshape(inst.n, -1, 32))
    got = waters11.encrypt_batch(TensorEngine(eng), f["g1a"], f["e_alpha"], f["h"], inst.policies, tm, ts, tv, tr)
    assert all(same_on_tensors(g, np.asarray(w)) for g, w in zip(got, want))


def test_keygen_batch_is_the_fixture_key_construction(setup):
    """three users with 4, 1 and 0 attributes: K = g1^(alpha + a t), L = g2^t, K_u = g1^(tau_u t), padded with the point at infinity"""
    eng, inst, f = setup
    a, alpha = fsc("a"), fsc("alpha")
    users = [[500, 11, 204, 22], [999], []]
    t = [fsc("t"), fsc("t", 1), fsc("t", 2)]
    K, L, kx, attrs = waters11.keygen_batch(eng, f["g1_alpha"], f["g1a"], f["h"], users, t)
    assert K.shape == (3, 64) and L.shape == (3, 128) and kx.shape == (3, 4, 64) and attrs.tolist() == [[11, 22, 204, 500], [999, -1, -1, -1], [-1] * 4]
    assert np.asarray(K).tobytes() == np.asarray(eng.g1_scalar_mul(G1, [(alpha + a * tj) % R for tj in t])).tobytes()
    assert np.asarray(L).tobytes() == np.asarray(eng.g2_scalar_mul(G2, list(t))).tobytes()
    for j, u in enumerate(users):
        want = np.asarray(eng.g1_scalar_mul(G1, [fsc("tau", x) * t[j] % R for x in sorted(u)])).reshape(-1, 64) if u else np.zeros((0, 64), np.uint8)
        assert np.asarray(kx)[j, :len(u)].tobytes() == want.tobytes() and not np.asarray(kx)[j, len(u):].any()
    # user 0 with the fixture's own t holds the fixture's key for those attributes
    assert K[0].tobytes() == inst.key[0].tobytes() and L[0].tobytes() == inst.key[1].tobytes()
    assert all(np.asarray(kx)[0, i].tobytes() == inst.key[2][u].tobytes() for i, u in enumerate([11, 22, 204, 500]))
    # ... and the key it returns decrypts: the first three policies need 11 and 22 / three of 200.. / 500
    key = (np.asarray(K)[0], np.asarray(L)[0], {int(u): np.asarray(kx)[0, i] for i, u in enumerate(attrs[0]) if u >= 0})
    out, ok = waters11.decrypt_batch(eng, key, inst.policies, inst.c, inst.c_prime, inst.cx, inst.dx)
    assert ok.tolist() == [1, 0, 1, 0] and np.asarray(out)[0].tobytes() == np.asarray(inst.msgs).reshape(-1, 384)[0].tobytes()
    tt = tensors(kbytes(t).reshape(-1, 32))[0]
    got = waters11.keygen_batch(TensorEngine(eng), f["g1_alpha"], f["g1a"], f["h"], users, tt)
    assert all(same_on_tensors(g.contiguous(), np.ascontiguousarray(w)) for g, w in zip(got[:3], (K, L, kx)))


def test_attributes_outside_the_universe_and_argument_errors(setup):
    eng, inst, f = setup
    msgs = np.asarray(inst.msgs)
    short = {u: p for u, p in f["h"].items() if u != 22}
    enc = lambda **kw: waters11.encrypt_batch(eng, f["g1a"], f["e_alpha"], kw.get("h", f["h"]), inst.policies, kw.get("msgs", msgs), kw.get("s", f["s"]), kw.get("v", f["v"]), kw.get("r", f["r"]),
                                             table=kw.get("table"))
    n_tables = len(eng.tables)
    with pytest.raises(ValueError, match="attribute 22 is not in the universe"):
        enc(h=short)
    with pytest.raises(ValueError, match="attribute 7 is not in the universe"):
        waters11.keygen_batch(eng, f["g1_alpha"], f["g1a"], f["h"], [[11], [7]], [1, 2])
    assert len(eng.tables) == n_tables                                                   # refused before the engine is touched
    small = waters11.encrypt_table(eng, f["g1a"], short)
    for bad in (lambda: enc(s=f["s"][:2]), lambda: enc(v=[row[:-1] for row in f["v"]]), lambda: enc(r=[row[:-1] for row in f["r"]]), lambda: enc(msgs=msgs.reshape(-1)[:-1]),
                lambda: enc(table=small), lambda: waters11.keygen_batch(eng, f["g1_alpha"], f["g1a"], f["h"], [[11, 11]], [1]),
                lambda: waters11.keygen_batch(eng, f["g1_alpha"], f["g1a"], f["h"], [[11]], [1, 2]),
                lambda: waters11.keygen_batch(eng, f["g1_alpha"][:32], f["g1a"], f["h"], [[11]], [1])):
        with pytest.raises(ValueError):
            bad()
