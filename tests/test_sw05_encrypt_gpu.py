"""SW05 SetUp / Encrypt of both universes, KeyGenerate by lookup and the d + 1 pair Decrypt on the MI355X (run with -m gpu) through
gopairingbasedcryptography_amd/sw05.py on the GPU engine and CUDA tensors: the cases and the expectations of tests/sw05_encrypt_cases.py
(the trapdoor exponents through the CPU oracle, the reference's loops written out), the round trip through the existing decrypt_batch /
decrypt_batch_large, FixedBase.msm over a table whose base 1 is the all-zero point, and Universe.lookup on 2^12 rows over 1500 values —
more than fr_find_common's 1024 — against a Python dict."""
import numpy as np
import pytest

import bn254_py as o
import chacha_cases as cc
import sw05_encrypt_cases as cases
from sw05_fixture import kbytes, sc
from test_sw05_encrypt_plan import KINDS, raw_rows3, rows3
from gopairingbasedcryptography_amd import rng, sw05

pytestmark = pytest.mark.gpu
R = o.R
SEED = bytes((31 * i + 5) % 256 for i in range(32))
OK8 = np.array(cases.OK, dtype=np.uint8)


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def dev(*arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda() for a in arrays]
    return out[0] if len(out) == 1 else out


def back(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def same(got, want):
    return all(back(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("kind", KINDS)
def test_small_universe_setup_encrypt_keygen_decrypt(oracle, eng, kind):
    u = cases.universe(sw05, kind)
    y, t, s, _ = cases.secrets(kind)
    T, Y, wantE, want_ep, msgs = cases.trapdoor_small(oracle, kind)
    gt_e = eng.GTFixedBase(cases.pairing(oracle).reshape(1, 384))
    pp, msk = sw05.setup(eng, u, *dev(kbytes([y]), kbytes(t)))
    assert pp["T"].is_cuda and same((pp["T"], pp["Y"], msk["y"], msk["t"]), (T, Y, kbytes([y]), kbytes(t)))
    hpp, _ = sw05.setup(eng, u, y, t, gt_table=gt_e)                                    # host arrays, Y from the table
    assert isinstance(hpp["T"], np.ndarray) and same((hpp["T"], hpp["Y"]), (T, Y))
    gt_e.close()
    attrs = cases.ct_attrs(kind)
    args = dev(raw_rows3(attrs), msgs, kbytes(s))
    E, e_prime, ok = sw05.encrypt_batch(eng, u, pp, *args)
    assert E.is_cuda and tuple(E.shape) == (5, 3, 128) and back(ok).tolist() == cases.OK == [1, 1, 0, 1, 1]
    assert same((E, e_prime), (wantE, want_ep))
    table, gt_y = sw05.encrypt_table(eng, pp), eng.GTFixedBase(pp["Y"].reshape(1, 384))
    assert same(sw05.encrypt_batch(eng, u, pp, *args, table=table, gt_table=gt_y), (wantE, want_ep, OK8))
    assert same(sw05.encrypt_batch(eng, u, hpp, attrs, msgs, s), (wantE, want_ep, OK8))          # host arrays, Python ints
    table.close(), gt_y.close()
    users = [cases.key_attrs(kind), [4, 78, 3], [9 + R, 5, cases.OWN[kind]]]
    coeffs = [[sc("kgu-%s" % kind, j)] for j in range(3)]
    D, kok = sw05.keygen_batch_universe(eng, u, msk, *dev(rows3(coeffs), raw_rows3(users)))
    pos = {v: i for i, v in enumerate(cases.MEMBERS[kind])}
    want_D = cases.g1_powers(oracle, [(y + coeffs[j][0] * a) * pow(t[pos[a % R]], -1, R) for j in (0, 2) for a in users[j]]).reshape(2, 3, 64)
    assert back(kok).tolist() == [1, 0, 1] and back(D)[[0, 2]].tobytes() == want_D.tobytes() and not back(D)[1].any()
    out, dok = sw05.decrypt_batch(eng, (users[0], back(D)[0]), cases.D, attrs, E, e_prime)
    want = cases.decryptable(kind)
    assert back(dok).tolist() == [int(w) for w in want] == [1, 0, 0, 1, 1]
    for c, w in enumerate(want):
        assert (back(out)[c] == msgs[c]).all() if w else not back(out)[c].any(), c


@pytest.mark.parametrize("which", ["reference", "paper"])
def test_large_universe_setup_encrypt_and_both_decrypts(oracle, eng, monkeypatch, which):
    n = cases.N_LARGE
    y, tau, s, _ = cases.secrets_large()
    t_of = cases.t_literal if which == "reference" else cases.t_paper
    wantE, want_pp, want_ep, msgs = cases.trapdoor_large(oracle, t_of)
    pp, msk = sw05.setup_large(eng, n, *dev(kbytes([y]), kbytes(tau)))
    assert same((pp["t"], pp["Y"], msk["y"]), (cases.g2_powers(oracle, tau), cases.gt_powers(oracle, [y])[0], kbytes([y])))
    table, nodes = sw05.large_table(eng, pp, nodes=None if which == "reference" else "paper")
    attrs = cases.LARGE_ATTRS
    args = dev(raw_rows3(attrs), msgs, kbytes(s))
    for route in ("dedupe", "fold", "auto"):
        assert same(sw05.encrypt_batch_large(eng, table, n, pp, *args, nodes=nodes, route=route), (wantE, want_pp, want_ep)), route
    monkeypatch.setattr(sw05, "FOLD_SCALAR_BYTES", 2 * (n + 2) * 32)                    # the fold route two rows at a time
    gt_y = eng.GTFixedBase(pp["Y"].reshape(1, 384))
    E, e_pp, e_prime = sw05.encrypt_batch_large(eng, table, n, pp, *args, nodes=nodes, route="fold", gt_table=gt_y)
    assert same((E, e_pp, e_prime), (wantE, want_pp, want_ep))
    monkeypatch.undo()
    gt_y.close()
    hpp = {"n": n, "t": back(pp["t"]), "Y": back(pp["Y"])}
    assert same(sw05.encrypt_batch_large(eng, table, n, hpp, attrs, msgs, s, nodes=nodes, route="fold"), (wantE, want_pp, want_ep))      # host arrays
    table.close()
    key = cases.large_key(oracle, t_of)
    out, ok = sw05.decrypt_batch_large(eng, key, cases.D, attrs, E, e_pp, e_prime)
    out_m, ok_m = sw05.decrypt_batch_large_msm(eng, key, cases.D, attrs, E, e_pp, e_prime)
    assert back(ok).tolist() == back(ok_m).tolist() == [int(w) for w in cases.LARGE_DECRYPTABLE] and back(out_m).tobytes() == back(out).tobytes()
    for c, w in enumerate(cases.LARGE_DECRYPTABLE):
        assert (back(out)[c] == msgs[c]).all() if w else not back(out)[c].any(), c
    rows_m = sw05.decrypt_batch_large_msm(eng, (dev(rows3([key[0]])[0]), dev(key[1]), dev(key[2])), cases.D, args[0], E, e_pp, e_prime)      # the rows form
    assert back(rows_m[0]).tobytes() == back(out).tobytes() and back(rows_m[1]).tolist() == back(ok).tolist()


def test_fixed_base_msm_with_an_all_zero_base(oracle, eng):
    """the reference's table [g2, infinity, t_1 .. t_3]: the base at position 1 contributes nothing, whatever its scalar"""
    taus = [sc("inf-tau", j) for j in range(3)]
    bases = np.concatenate([cases.G2.reshape(1, 128), np.zeros((1, 128), dtype=np.uint8), cases.g2_powers(oracle, taus)])
    rows = [[sc("inf-k", 5 * i + j) for j in range(5)] for i in range(6)]
    rows[1][1], rows[2], rows[3] = 0, [0, 7, 0, 0, 0], [0, 0, 0, 0, 0]                  # a zero scalar on it; it alone; nothing at all
    want = np.stack([np.asarray(oracle.g2_sum(oracle.g2_scalar_mul(bases.reshape(-1), kbytes(r)))).reshape(128) for r in rows])
    assert want[0].any() and not want[2].any() and not want[3].any()
    assert want[0].tobytes() == cases.g2_powers(oracle, [rows[0][0] + sum(k * t for k, t in zip(rows[0][2:], taus))]).tobytes()      # and through the exponent
    for put in (lambda a: a, dev):
        table = eng.FixedBase(put(bases), g2=True)
        assert back(table.msm(put(kbytes([k for r in rows for k in r])))).tobytes() == want.tobytes()
        table.close()


def test_lookup_of_4096_rows_over_1500_values(eng):
    values = [sc("gu", i) if i % 4 == 0 else 5000 + 3 * i for i in range(1500)]
    for u, members in ((sw05.Universe.from_values(values + values[:9]), values), (sw05.Universe.range(-700, 800), [v % R for v in range(-700, 800)]),
                       (sw05.Universe.range(40, 1540), list(range(40, 1540)))):
        assert u.size == 1500
        where = {v: i for i, v in enumerate(members)}
        queries = [[members[(7 * c + 411 * j) % 1500] if (c + j) % 3 else sc("gq", 4 * c + j) + (R if c % 5 == 0 else 0) for j in range(4)] for c in range(1024)]
        queries[3], queries[5][2] = [members[j] + R for j in range(4)], R + 3000        # members written as x + r; 3000 is in no universe here
        index, ok = u.lookup(eng, dev(raw_rows3(queries)))
        assert index.is_cuda and str(index.dtype) == "torch.int32" and tuple(index.shape) == (1024, 4)
        want = [[where.get(a % R, sw05.INDEX_NONE) for a in row] for row in queries]
        assert back(index).view(np.uint32).tolist() == want
        assert back(ok).tolist() == [int(all(v != sw05.INDEX_NONE for v in row)) for row in want] and back(ok)[3] == 1
        host_index, host_ok = u.lookup(eng, raw_rows3(queries[:64]))                    # host arrays through the same engine
        assert host_index.tolist() == want[:64] and host_ok.tolist() == back(ok)[:64].tolist()


def test_seeded_forms_are_the_unseeded_calls_on_the_scalars_drawn(oracle, eng):
    u = cases.universe(sw05, "int64")
    like = dev(np.zeros(0, dtype=np.uint8))
    rs = rng.Randomness(eng, SEED)
    pp, msk = sw05.setup_seeded(eng, u, rs, like=like)
    assert rs.next_stream == 2 and pp["T"].is_cuda
    want_pp, want_msk = sw05.setup(eng, u, cc.scalars(SEED, 1, 0, 1), cc.scalars(SEED, 0, 0, 7))      # t [U] first, then y
    assert same((pp["T"], pp["Y"], msk["y"], msk["t"]), (want_pp["T"], want_pp["Y"], want_msk["y"], want_msk["t"]))
    msgs = dev(cases.gt_powers(oracle, [5, 6, 7, 8, 9]))
    attrs = cases.ct_attrs("int64")
    got = sw05.encrypt_batch_seeded(eng, u, pp, attrs, msgs, rs)
    assert rs.next_stream == 3 and same(got, [back(x) for x in sw05.encrypt_batch(eng, u, pp, attrs, msgs, dev(cc.scalars(SEED, 2, 0, 5)))])
    n = cases.N_LARGE
    rs = rng.Randomness(eng, SEED)
    lpp, lmsk = sw05.setup_large_seeded(eng, n, rs, like=like)
    want_l, want_m = sw05.setup_large(eng, n, cc.scalars(SEED, 0, 0, 1), cc.scalars(SEED, 1, 0, n + 1))      # y first, then tau
    assert same((lpp["t"], lpp["Y"], lmsk["y"]), (want_l["t"], want_l["Y"], want_m["y"]))
    table, nodes = sw05.large_table(eng, lpp)
    got = sw05.encrypt_batch_large_seeded(eng, table, n, lpp, cases.LARGE_ATTRS, msgs, rs, nodes=nodes)
    want = sw05.encrypt_batch_large(eng, table, n, lpp, cases.LARGE_ATTRS, msgs, dev(cc.scalars(SEED, 2, 0, 5)), nodes=nodes, route="fold")
    assert rs.next_stream == 3 and same(got, [back(x) for x in want])
    table.close()
