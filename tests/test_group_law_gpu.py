"""Elementwise group law on the MI355X (run with -m gpu): k_g1_add .. k_g2_dbl through the host-pointer and the device entries.

  * oracle parity: random pairs, every special case at every position of an inversion group, a broadcast b, sizes 1, K-1, K+1
    and 1000, in place (out = a; out = b with one b per a), against the Python oracle bit for bit;
  * 2^20 algebraic check, independent of the new kernels: A_i = [a_i]g, B_i = [b_i]g by the engine's scalar multiplication, then
    A + B = [a + b]g, A - B = [a - b]g, 2A = [2a]g (scalars mod r), with infinity, b = a and b = -a at the edges of inversion
    groups, wavefronts and shards; device entries, then host entries in a process bound to the device list {0, 0} (the shard
    split is crossed) including one call on the own-lane route; a 4096-element sample against the Python oracle;
  * scheme pipelines kept in HBM: ZSS04 verification of 64 signatures, BSW07's D_j = [r]g2 + [r_j]H_j for 256 attributes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bn254_py as o
from conftest import ROOT
from group_law_cases import ADD, DBL, GROUPS, OPS, SPECIALS, SUB, algebraic_scalars, special_batch, special_positions

pytestmark = pytest.mark.gpu
KS = {"g1": 6, "g2": 8}                  # GROUP_K_G1 / _G2 of csrc/group29.hip.hpp (tests/test_group_law.py reads them from the harness)


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def fns(eng, name):
    return {ADD: getattr(eng, name + "_add"), SUB: getattr(eng, name + "_sub"), DBL: getattr(eng, name + "_double")}


def call(f, op, a, b, out=None):
    return f[op](a, out=out) if op == DBL else f[op](a, b, out=out)


def cases(grp, oracle, name):
    """(label, op, A, B) of the oracle-parity list"""
    K = KS[name]
    out = []
    for op in OPS:
        for n in (1, K - 1, K + 1, 1000):
            out.append(("rand%d" % n, op, grp.points(oracle, "gpu-a%d-%d" % (op, n), n), grp.points(oracle, "gpu-b%d-%d" % (op, n), n)))
    for op, kind in [(op, kind) for op in (ADD, SUB) for kind in SPECIALS] + [(DBL, "a_inf")]:
        A, B = special_batch(grp, oracle, op, kind, K, "gpu-sp-%s-%d-%s" % (name, op, kind))
        out.append((kind, op, A, B))
    A, B = grp.points(oracle, "gpu-bc-a-" + name, 5 * K + 3), grp.points(oracle, "gpu-bc-b-" + name, 1)
    A[3] = B[0]
    A[K + 1] = grp.neg_rows(B)[0]
    A[2 * K] = 0
    for op in (ADD, SUB):
        out.append(("broadcast", op, A, B))
        out.append(("broadcast-inf", op, A, np.zeros_like(B)))
    return out


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_oracle_parity_host_and_device(eng, oracle, name):
    import torch
    grp = GROUPS[name]
    f = fns(eng, name)
    for label, op, A, B in cases(grp, oracle, name):
        want = grp.expect(op, A, B)
        got = call(f, op, A, B)
        assert (got == want).all(), ("host", name, label, op, np.nonzero((got != want).any(axis=1))[0][:8])
        tA, tB = torch.from_numpy(A.copy()).cuda(), torch.from_numpy(B.copy()).cuda()
        got = call(f, op, tA, tB).cpu().numpy()
        assert (got == want).all(), ("dev", name, label, op, np.nonzero((got != want).any(axis=1))[0][:8])
        # in place: out = a, and out = b when b has one row per a (gnark's p.Add(p, q))
        Ai = A.copy()
        call(f, op, Ai, B, out=Ai)
        assert (Ai == want).all(), ("host out=a", name, label, op)
        tAi = tA.clone()
        call(f, op, tAi, tB, out=tAi)
        assert (tAi.cpu().numpy() == want).all(), ("dev out=a", name, label, op)
        if op != DBL and B.shape[0] == A.shape[0]:
            Bi = B.copy()
            call(f, op, A, Bi, out=Bi)
            assert (Bi == want).all(), ("host out=b", name, label, op)
            tBi = tB.clone()
            call(f, op, tA, tBi, out=tBi)
            assert (tBi.cpu().numpy() == want).all(), ("dev out=b", name, label, op)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_algebraic_2_20(eng, oracle, name, tmp_path):
    """2^20 elements: A + B, A - B, 2A against [a + b]g, [a - b]g, [2a]g from the engine's scalar multiplication (the parent
    commit's code, untouched) — device entries here, host entries in a process of their own over the device list {0, 0}"""
    import torch
    n = 1 << 20
    grp = GROUPS[name]
    f = fns(eng, name)
    g2 = name == "g2"
    smul = eng.g2_scalar_mul if g2 else eng.g1_scalar_mul
    gen = torch.from_numpy(eng.generators()[1 if g2 else 0].copy()).cuda()
    pos, ks = algebraic_scalars(n, KS[name], 2020 + g2)
    pts = {k: smul(gen, torch.from_numpy(v.reshape(-1)).cuda()) for k, v in ks.items()}
    A, B = pts.pop("a"), pts.pop("b")
    zero_a = torch.nonzero((A == 0).all(dim=1)).flatten().cpu().numpy()
    assert set(zero_a.tolist()) >= {pos[i] for i in range(0, len(pos), 5)}          # the scalar 0 gave infinity where it was put
    for label, got, want in (("add", f[ADD](A, B), pts["sum"]), ("sub", f[SUB](A, B), pts["diff"]), ("dbl", f[DBL](A), pts["dbl"])):
        wrong = torch.nonzero((got != want).any(dim=1)).flatten()
        print(name, label, "device entries: %d of %d rows differ" % (wrong.numel(), n))
        assert wrong.numel() == 0, (label, wrong[:8].tolist())
    # a 4096-element sample (the special positions first) against the Python oracle
    rng = np.random.default_rng(7)
    sample = np.concatenate([np.array(pos), np.setdiff1d(rng.choice(n, 8192, replace=False), pos)[:4096 - len(pos)]])
    An, Bn = A.cpu().numpy(), B.cpu().numpy()
    for label, op, res in (("add", ADD, pts["sum"]), ("sub", SUB, pts["diff"]), ("dbl", DBL, pts["dbl"])):
        want = grp.expect(op, An[sample], Bn[sample])
        assert (res.cpu().numpy()[sample] == want).all(), (name, label)
    # host entries over two device slots (the shard split at n / 2 is a special position) and one own-lane call
    np.savez(tmp_path / "in.npz", A=An, B=Bn, **{k: pts[k].cpu().numpy() for k in ("sum", "diff", "dbl")})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "group_law_cases.py"), str(tmp_path / "in.npz"), name, "0", "0"],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "devices 2 failures []" in r.stdout


def test_zss04_verification_in_hbm(eng, oracle):
    """ZSS04: sigma_i = [1 / (h_i + x)]g1, pk = [x]g2 (oracle).  On the device: [h_i]g2, + pk (one b for all), and the two-pair
    products e(sigma_i, [h_i]g2 + pk) e(-g1, g2) == 1 — all 64 true, a corrupted sigma false."""
    import torch
    n = 64
    g1, g2 = eng.generators()
    x = o.bench_scalar("zss04-x", 0) % o.R
    h = [o.bench_scalar("zss04-h", i) % o.R for i in range(n)]
    inv = [pow((hi + x) % o.R, -1, o.R) for hi in h]
    rows = lambda ks: np.frombuffer(b"".join(k.to_bytes(32, "little") for k in ks), dtype=np.uint8).copy()
    sigma = np.asarray(oracle.g1_scalar_mul(g1, rows(inv))).reshape(n, 64)
    pk = np.asarray(oracle.g2_scalar_mul(g2, rows([x]))).reshape(1, 128)
    dev = lambda a: torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()
    Hm = eng.g2_scalar_mul(dev(g2), dev(rows(h)))
    Q = eng.g2_add(Hm, dev(pk))
    ng1 = dev(eng.g1_neg(g1)).reshape(1, 64)
    seg = np.arange(0, 2 * n + 1, 2, dtype=np.uint64)
    one = dev(np.frombuffer(o.gt_to_bytes(o.F12_ONE), dtype=np.uint8)).reshape(1, 384)

    def verify(S):
        P2 = torch.stack([S, ng1.expand(n, 64)], dim=1).reshape(2 * n, 64).contiguous()
        Q2 = torch.stack([Q.reshape(n, 128), dev(g2).reshape(1, 128).expand(n, 128)], dim=1).reshape(2 * n, 128).contiguous()
        return (eng.multi_pair(P2, Q2, seg) == one).all(dim=1).cpu().numpy()

    S = dev(sigma)
    assert verify(S).all()
    S[5] = S[6]
    ok = verify(S)
    assert not ok[5] and ok.sum() == n - 1


def test_bsw07_key_components_in_hbm(eng, oracle):
    """BSW07 KeyGen: D_j = [r]g2 + [r_j]H_j for 256 attributes, scalar multiplications and the broadcast addition on the device"""
    import torch
    n = 256
    g1, g2 = eng.generators()
    rows = lambda ks: np.frombuffer(b"".join((k % o.R).to_bytes(32, "little") for k in ks), dtype=np.uint8).copy()
    H = np.asarray(oracle.g2_scalar_mul(g2, rows([o.bench_scalar("bsw07-H", j) for j in range(n)]))).reshape(n, 128)
    rj = rows([o.bench_scalar("bsw07-rj", j) for j in range(n)])
    r = rows([o.bench_scalar("bsw07-r", 0)])
    dev = lambda a: torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()
    D = eng.g2_add(eng.g2_scalar_mul(dev(H), dev(rj)), eng.g2_scalar_mul(dev(g2), dev(r)))
    want = GROUPS["g2"].expect(ADD, np.asarray(oracle.g2_scalar_mul(H, rj)).reshape(n, 128), np.asarray(oracle.g2_scalar_mul(g2, r)).reshape(1, 128))
    assert (D.cpu().numpy() == want).all()


def test_special_positions_cover_the_edges():
    """the 2^20 check puts its special elements on every position of lane 0's and the last lane's groups, on both sides of a
    wavefront edge and of the shard split"""
    n = 1 << 20
    for K in KS.values():
        T = (n + K - 1) // K
        p = set(special_positions(n, K))
        assert all(j * T in p and min(j * T + T - 1, n - 1) in p and j * T + 63 in p and j * T + 64 in p for j in range(K))
        assert {n // 2 - 1, n // 2, n - 1} <= p
