"""The scalar field Fr on the MI355X (run with -m gpu): k_fr_* through the host-pointer and the device entries.

  * the case lists of tests/fr_cases.py (edge values, zeros at every position of an inversion group, broadcast b, sizes, in
    place; both polynomial kernels for every B of the list) against Python's integers, host arrays and CUDA tensors, and once
    more in a process bound to the device list {0, 0} with batches large enough to cross the shard split;
  * 2^20 elements checked by identities that do not rest on the new kernels alone;
  * chaining: the ZSS04 exponents 1 / (H(m) + x) made on the device and fed to the fixed-base table as device scalars;
  * AFP25 from identities and SRS on the small fixture (B = 6, B = 64) and at BASELINE config 5's stated size, 2^18 items in
    batches of 256: every digest, every opening proof (against the instance's, which were derived from the trapdoor tau by one
    modular inversion: a route that shares nothing with the polynomial kernels) and every message."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bn254_py as o
from conftest import ROOT
import fr_cases as fc
from gopairingbasedcryptography_amd import afp25

pytestmark = pytest.mark.gpu
FR_INV_K = 8                                   # csrc/fr29.hip.hpp (tests/test_fr.py reads it from the harness)


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 6. the case lists
def test_elementwise_cases_host_and_device(eng):
    import torch
    assert fc.run_engine_cases(eng, FR_INV_K) == []
    assert fc.run_engine_cases(eng, FR_INV_K, dev=to_dev) == []
    torch.cuda.synchronize()


def test_polynomial_cases_host_and_device(eng):
    import torch
    assert fc.ints(eng.fr_poly_from_roots([[1, 2]])) == [2, fc.R - 3, 1]
    assert fc.run_engine_poly(eng, fc.POLY_BS) == []
    assert fc.run_engine_poly(eng, fc.POLY_BS, dev=to_dev) == []
    torch.cuda.synchronize()


def test_quotients_into_caller_buffers_on_device(eng):
    """out= / ok= on CUDA tensors: the kernel fills exactly the caller's rows (a guard row behind them stays as it was)"""
    import torch
    B, stride = 65, 66
    polys = fc.poly_cases(B)
    coeffs, points, want = fc.quotient_case(polys, B)
    n = len(want)
    buf = torch.full(((n + 1) * stride * 32,), 0x5A, dtype=torch.uint8, device="cuda")
    okb = torch.full((n + 1,), 0x5A, dtype=torch.uint8, device="cuda")
    q, ok = eng.fr_poly_quotients(to_dev(fc.rows([c for f in coeffs for c in f]).reshape(-1)), to_dev(fc.rows([x for p in points for x in p]).reshape(-1)),
                                  B, stride, out=buf[:n * stride * 32], ok=okb[:n])
    assert fc.check_quotients(q.cpu().numpy(), ok.cpu().numpy(), want, B, stride) == []
    assert bool((buf[n * stride * 32:] == 0x5A).all()) and int(okb[n]) == 0x5A


def test_host_entries_across_the_shard_split():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fr_cases.py"), "0", "0"], capture_output=True, text=True, timeout=900)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "devices 2 failures []" in r.stdout


# ------------------------------------------------------------------------------------------------ 7. 2^20 elements
def test_identities_2_20(eng, oracle):
    import torch
    n = 1 << 20
    rng = np.random.default_rng(2025)
    raw = rng.integers(0, 1 << 32, size=(2, n, 8), dtype=np.uint64).astype(np.uint32)
    raw[0, :, 7] &= 0x1FFFFFFF                                     # a < 2^253 < r: canonical already; b is any 256-bit value
    T = (n + FR_INV_K - 1) // FR_INV_K
    zeros = sorted({j * T + off for j in range(FR_INV_K) for off in (0, 1, 63, 64, T - 1) if j * T + off < n} | {n // 2, n - 1})
    A, Bv = raw[0].view(np.uint8).reshape(n, 32).copy(), raw[1].view(np.uint8).reshape(n, 32).copy()
    A[zeros] = 0
    a, b = to_dev(A), to_dev(Bv)
    one = to_dev(fc.rows([1]))
    inv = eng.fr_inverse(a)
    prod = eng.fr_mul(inv, a)
    is_zero = torch.zeros(n, dtype=torch.bool, device="cuda")
    is_zero[torch.tensor(zeros, device="cuda")] = True
    wrong = torch.nonzero(((prod != one).any(dim=1) & ~is_zero) | ((prod != 0).any(dim=1) & is_zero) | ((inv != 0).any(dim=1) & is_zero)).flatten()
    print("inverse(a) a == 1: %d of %d rows differ" % (wrong.numel(), n))
    assert wrong.numel() == 0, wrong[:8].tolist()
    back = eng.fr_sub(eng.fr_add(a, b), b)
    wrong = torch.nonzero((back != a).any(dim=1)).flatten()
    print("(a + b) - b == a: %d of %d rows differ" % (wrong.numel(), n))
    assert wrong.numel() == 0, wrong[:8].tolist()
    assert bool((eng.fr_from_mont(eng.fr_to_mont(a)) == a).all()) and bool((eng.fr_neg(eng.fr_neg(a)) == a).all())
    ab = eng.fr_mul(a, b)
    sample = np.concatenate([np.array(zeros), np.setdiff1d(rng.choice(n, 8192, replace=False), zeros)[:4096 - len(zeros)]])
    ai, bi = fc.ints(A[sample]), fc.ints(Bv[sample])
    assert fc.ints(ab.cpu().numpy()[sample]) == [x * y % fc.R for x, y in zip(ai, bi)]
    assert fc.ints(inv.cpu().numpy()[sample]) == fc.expect("inverse", ai)
    # [a b]g1 == [a]([b]g1) through the engine's scalar multiplication (the parent commit's code)
    st = to_dev(sample)
    g1 = to_dev(eng.generators()[0].copy())
    lhs = eng.g1_scalar_mul(g1, ab[st].contiguous())
    rhs = eng.g1_scalar_mul(eng.g1_scalar_mul(g1, b[st].contiguous()), a[st].contiguous())
    assert bool((lhs == rhs).all())


# ------------------------------------------------------------------------------------------------ 8. chaining
def test_zss04_signatures_from_device_scalars(eng, oracle):
    """sigma_i = [1 / (H(m_i) + x)]g1 for 1024 messages: the exponent by fr_add (one x for all) and fr_inverse on CUDA tensors, the
    generator multiplication from the HBM table with those tensors as its scalars; equal to the oracle's signatures"""
    n = 1024
    g1 = eng.generators()[0]
    x = o.bench_scalar("zss04-x", 0)
    h = [o.bench_scalar("zss04-h", i) for i in range(n)]
    h[7] = (-x) % o.R                                              # H(m) + x = 0: gnark's Inverse gives 0, the signature is infinity
    want_k = [pow((hi + x) % o.R, -1, o.R) if (hi + x) % o.R else 0 for hi in h]
    want = np.asarray(oracle.g1_scalar_mul(g1, fc.rows(want_k).reshape(-1))).reshape(n, 64)
    k = eng.fr_inverse(eng.fr_add(to_dev(fc.rows(h)), to_dev(fc.rows([x]))))
    assert fc.ints(k.cpu().numpy()) == want_k
    table = eng.FixedBase(g1)
    try:
        sigma = table.mul(k.reshape(-1))
    finally:
        table.close()
    assert (sigma.cpu().numpy() == want).all() and not want[7].any()


# ------------------------------------------------------------------------------------------------ 9. AFP25 on the fixture
def encrypt_for(inst, eng, ident, t):
    """one more item for `ident`, as tests/afp25_fixture.Instance makes them (the fixture covers only some identities of a batch)"""
    from afp25_fixture import sc
    msk, tau = sc("msk"), sc("tau")
    g2_tau, g2_msk = eng.g2_scalar_mul(inst.g2, [tau])[0], eng.g2_scalar_mul(inst.g2, [msk])[0]
    ht = eng.g1_scalar_mul(inst.g1, [sc("ht")])[0]
    r1, r2 = sc("r1", 1000 + t), sc("r2", 1000 + t)
    M = eng.gt_exp(eng.pair_batch(inst.g1, inst.g2), [sc("msg", 1000 + t)])[0]
    c10 = eng.g2_sum(np.concatenate([eng.g2_scalar_mul(inst.g2, [r1])[0], eng.g2_scalar_mul(g2_msk, [r2])[0]]))
    a01 = eng.g2_sum(np.concatenate([eng.g2_scalar_mul(inst.g2, [ident])[0], eng.g2_scalar_mul(g2_tau, [o.R - 1])[0]]))
    c11, c12 = eng.g2_scalar_mul(a01, [r1])[0], eng.g2_scalar_mul(inst.g2, [(-r2) % o.R])[0]
    c2 = eng.gt_mul(eng.gt_exp(eng.pair_batch(ht, g2_msk), [(-r2) % o.R]), M)[0]
    return (ident, np.stack([np.asarray(c10), np.asarray(c11), np.asarray(c12)]), np.asarray(c2)), np.asarray(M)


@pytest.mark.parametrize("B", [6, 64])
def test_afp25_fixture_from_identities(eng, oracle, B):
    from afp25_fixture import Instance
    inst = Instance(eng, B, B)
    by_ident = {}
    for item, msg in zip(inst.items, inst.msgs):
        by_ident.setdefault(item[0], (item, msg))
    assert B != 64 or len(by_ident) == 64                          # (3t + 1) mod 64 reaches every identity
    items, msgs = [], []
    for i, ident in enumerate(inst.ids):
        item, msg = by_ident[ident] if ident in by_ident else encrypt_for(inst, eng, ident, i)
        items.append(item)
        msgs.append(msg)
    table = afp25.srs_table(eng, inst.g1, inst.tau_powers)
    try:
        want_pi = np.stack([np.asarray(afp25.commit_g1(eng, inst.g1, inst.tau_powers, afp25.quotient_by_root(inst.f, ident))).reshape(64) for ident in inst.ids])
        want_msgs = np.stack(msgs)
        ref = np.stack([np.asarray(inst.reference_shaped_decrypt(oracle, it)) for it in items])
        assert (want_msgs == ref).all()
        C1, C2 = np.stack([it[1] for it in items]), np.stack([it[2] for it in items])
        ids_rows = fc.rows(inst.ids)
        for ids, put in (([inst.ids], lambda x: x), (ids_rows, lambda x: x), (to_dev(ids_rows), to_dev)):
            back = (lambda x: x.cpu().numpy()) if put is to_dev else np.asarray
            assert (back(afp25.digests(eng, table, ids)) == np.asarray(inst.D).reshape(1, 64)).all()
            assert (back(afp25.opening_proofs(eng, table, ids)) == want_pi).all()
            got = back(afp25.decrypt_batches(eng, table, ids, put(np.asarray(inst.sk).reshape(1, 64)), put(C1), put(C2)))
            assert (got == want_msgs).all() and (got == ref).all()
        # two batches in one call (the same batch twice), a key per item, the digests handed in
        ids2 = to_dev(np.concatenate([ids_rows, ids_rows]))
        sk2 = to_dev(np.tile(np.asarray(inst.sk).reshape(1, 64), (2 * B, 1)))
        D2 = to_dev(np.tile(np.asarray(inst.D).reshape(1, 64), (2, 1)))
        got = afp25.decrypt_batches(eng, table, ids2, sk2, to_dev(np.concatenate([C1, C1])), to_dev(np.concatenate([C2, C2])), D=D2).cpu().numpy()
        assert (got == np.concatenate([want_msgs, want_msgs])).all()
        # an identity that is not in its batch: no proof, an error
        wrong = ids_rows.copy()
        wrong[B // 2] = fc.rows([fc.non_root(inst.ids)])[0]
        coeffs = eng.fr_poly_from_roots(ids_rows.reshape(-1), B)
        with pytest.raises(ValueError):
            afp25.opening_proofs(eng, table, wrong, coeffs=coeffs)
    finally:
        table.close()


# ------------------------------------------------------------------------------------------------ 10. config 5 at its stated size
def test_config5_from_identities_2_18(eng):
    """2^18 items in 1024 batches of B = 256 from device-resident identities and the SRS table: every digest, every opening proof
    and every message, no sampling"""
    import torch
    import bench_workloads as w
    n, B = 1 << 18, 256
    dev = torch.device("cuda", 0)
    inst = w.afp25_instance(eng, B, n, dev)
    table = afp25.srs_table(eng, inst["g1"], w.afp25_srs(eng, inst))
    try:
        ids = to_dev(fc.rows(inst["ids"]))
        D = afp25.digests(eng, table, ids)
        wrong = torch.nonzero((D.reshape(n // B, 1, 64) != inst["D"].reshape(n // B, B, 64)).any(dim=2)).shape[0]
        print("digests: %d of %d item rows differ" % (wrong, n))
        assert wrong == 0
        pi = afp25.opening_proofs(eng, table, ids)
        wrong = torch.nonzero((pi != inst["pi"]).any(dim=1)).flatten()
        print("opening proofs: %d of %d differ" % (wrong.numel(), n))
        assert wrong.numel() == 0, wrong[:8].tolist()
        del pi
        out = afp25.decrypt_batches(eng, table, ids, inst["sk"], inst["C1"], inst["C2"])
        wrong = torch.nonzero((out != inst["msgs"]).any(dim=1)).flatten()
        print("messages: %d of %d differ" % (wrong.numel(), n))
        assert wrong.numel() == 0, wrong[:8].tolist()
    finally:
        table.close()
        eng.release_workspaces()
