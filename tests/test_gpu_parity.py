"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI, against
  * the committed golden vectors (tests/golden, made by the big-integer oracle), and
  * the C restatement (oracle/) on the same seeded inputs,
bit for bit.  Edge cases follow gnark's semantics at the boundary: infinity in either
slot -> GT one, scalar 0 / >= r, length mismatch -> "invalid inputs sizes"."""
import numpy as np
import pytest

import bn254_py as o
from conftest import cat, eip197_pairs, hx, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def scalars(tag, n, start=0):
    return np.frombuffer(b"".join(o.scalar_to_bytes(o.bench_scalar(tag, start + i)) for i in range(n)), dtype=np.uint8)


@pytest.fixture(scope="module")
def synth(eng, oracle):
    """P_i=[k('P',i)]g1, Q_i=[k('Q',i)]g2 made by the engine's scalar-mul kernels, checked against the oracle."""
    n = 192
    g1, g2 = eng.generators()
    P = eng.g1_scalar_mul(g1, scalars("P", n))
    Q = eng.g2_scalar_mul(g2, scalars("Q", n))
    assert (P == oracle.g1_scalar_mul(g1, scalars("P", n), threads=8)).all()
    assert (Q == oracle.g2_scalar_mul(g2, scalars("Q", n), threads=8)).all()
    return P, Q


def test_fp_mul_random(eng, oracle):
    rng = np.random.default_rng(254)
    n = 4096
    vals = [int.from_bytes(rng.bytes(32), "little") % o.P for _ in range(2 * n)]
    vals[0], vals[1], vals[2], vals[3] = 0, o.P - 1, 1, o.P - 1
    a = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals[:n]), dtype=np.uint8)
    b = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals[n:]), dtype=np.uint8)
    assert (eng.fp_mul(a, b) == oracle.fp_mul(a, b)).all()


def test_pairing_golden(eng):
    g = load_golden("pairing.json")["cases"]
    out = eng.pair_batch(cat([c["P"] for c in g]), cat([c["Q"] for c in g]))
    for i, c in enumerate(g):
        assert out[i].tobytes().hex() == c["GT"], c["note"]


def test_pairing_vs_oracle(eng, oracle, synth):
    P, Q = synth
    assert (eng.pair_batch(P, Q) == oracle.pair_batch(P, Q, threads=8)).all()


def test_stages_vs_oracle(eng, oracle, synth):
    P, Q = synth[0][:70], synth[1][:70]        # 70: a ragged tail wave (64 + 6)
    f = eng.miller_loop(P, Q)
    assert (eng.final_exp(f) == oracle.pair_batch(P, Q, threads=8)).all()
    # final exponentiation alone, fed the oracle's Miller values
    fo = oracle.miller_loop(P, Q, threads=8)
    assert (eng.final_exp(fo) == oracle.final_exp(fo, threads=8)).all()


def test_pair_single_call_semantics(eng):
    """bn254.Pair(P,Q) with len 1 and len>1, and its error on mismatched or empty input."""
    segs = load_golden("multi_pair.json")["segments"]
    s = segs[3]
    assert eng.pair(cat(s["P"]), cat(s["Q"])).tobytes().hex() == s["GT"]
    g1, g2 = eng.generators()
    with pytest.raises(ValueError, match="invalid inputs sizes"):
        eng.pair(np.concatenate([g1, g1]), g2)
    with pytest.raises(ValueError, match="invalid inputs sizes"):
        eng.pair(np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8))


def test_published_pairing_check_vector(eng):
    """The EIP-197 known answer (tests/golden/eip197_pairing.json; an external vector, see tests/test_oracle.py) through the engine:
    PairingCheck accepts it in the latency form and through the throughput kernels, and rejects it with another second point."""
    from gopairingbasedcryptography_amd import _lib
    for c in load_golden("eip197_pairing.json")["cases"]:
        ps, qs = eip197_pairs(c["words"])
        P = np.frombuffer(b"".join(o.g1_to_bytes(p) for p in ps), dtype=np.uint8)
        Q = np.frombuffer(b"".join(o.g2_to_bytes(q) for q in qs), dtype=np.uint8)
        Q2 = np.frombuffer(o.g2_to_bytes(qs[0]) + o.g2_to_bytes(o.g2_mul(o.G2_GEN, 2)), dtype=np.uint8)
        one = np.frombuffer(o.gt_to_bytes(o.F12_ONE), dtype=np.uint8)
        for limit in (2048, 0):
            _lib.check(_lib.load().gpbc_set_latency_path(limit))
            try:
                assert bool(eng.pairing_check(P, Q)) == c["expected"]
                assert not eng.pairing_check(P, Q2)
                assert (np.asarray(eng.pair(P, Q)).reshape(-1) == one).all() == c["expected"]
            finally:
                _lib.load().gpbc_set_latency_path(2048)


def test_multi_pair_golden(eng):
    segs = load_golden("multi_pair.json")["segments"]
    P = cat([h for s in segs for h in s["P"]]); Q = cat([h for s in segs for h in s["Q"]])
    off = np.cumsum([0] + [len(s["P"]) for s in segs])
    out = eng.multi_pair(P, Q, off)
    ok = eng.pairing_check_batch(P, Q, off)
    for i, s in enumerate(segs):
        assert out[i].tobytes().hex() == s["GT"], s["note"]
        assert bool(ok[i]) == s["is_one"], s["note"]


def test_multi_pair_ragged_vs_oracle(eng, oracle, synth):
    P, Q = synth
    lens = [0, 1, 7, 0, 64, 3, 65, 2, 33, 17]            # includes empty segments
    off = np.cumsum([0] + lens)
    n = int(off[-1])
    assert (eng.multi_pair(P[:n], Q[:n], off) == oracle.multi_pair(P[:n], Q[:n], off, threads=8)).all()


def test_multi_pair_shared_squarings_chunks(eng, oracle, synth):
    """Host multi_pair cuts segments into chunks of up to 8 pairs that share the Miller squarings: segment lengths around
    the chunk size, an empty segment, points at infinity in the first / middle / last position of a chunk and a whole
    chunk of infinities — against the C restatement, and against the product of single pairings."""
    P, Q = synth
    P, Q = P.reshape(-1, 64).copy(), Q.reshape(-1, 128).copy()
    lens = [1, 7, 8, 9, 40, 0, 33, 16]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(off[-1])
    P, Q = P[:n], Q[:n]
    P[off[2]] = 0                    # first pair of the 8-segment
    Q[off[3] + 4] = 0                # middle of a chunk
    P[off[3] + 7] = 0                # last of the first chunk of the 9-segment
    P[off[6]:off[6] + 16] = 0        # two whole chunks of infinities inside the 33-segment
    from gopairingbasedcryptography_amd import _lib
    want = oracle.multi_pair(P, Q, off, threads=8)
    try:
        for chunk in (8, 5, 1, 0):                     # forced chunk lengths, then the automatic choice
            _lib.check(_lib.load().gpbc_set_multi_pair_chunk(chunk))
            got = eng.multi_pair(P, Q, off)
            assert (got == want).all(), chunk
            import torch
            got_dev = eng.multi_pair(torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda(), off)      # host table, device points
            assert (got_dev.cpu().numpy() == want).all(), chunk
    finally:
        _lib.load().gpbc_set_multi_pair_chunk(0)
    single = eng.pair_batch(P, Q)
    for j, ln in enumerate(lens):
        acc = np.frombuffer(o.gt_to_bytes(o.F12_ONE), dtype=np.uint8)
        for i in range(int(off[j]), int(off[j + 1])):
            acc = eng.gt_mul(acc, single[i])[0]
        assert (got[j] == acc).all(), j
    ok = eng.pairing_check_batch(P, Q, off)
    assert ok.tolist() == [0, 0, 0, 0, 0, 1, 0, 0]          # only the empty product is one


def test_release_workspaces(eng, synth):
    """gpbc_release_workspaces hands the grow-only buffers back; the next calls rebuild them and give the same bytes."""
    import torch
    P, Q = synth
    P, Q = P.reshape(-1, 64)[:64], Q.reshape(-1, 128)[:64]
    dP, dQ = torch.from_numpy(P.copy()).cuda(), torch.from_numpy(Q.copy()).cuda()
    before = (eng.pair_batch(dP, dQ).cpu().numpy(), eng.multi_pair_fixed_q(P[:48].copy(), Q[:12].copy()), eng.g1_scalar_mul(P, scalars("rel", 64)))
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    eng.release_workspaces()
    assert torch.cuda.mem_get_info()[0] >= free0
    after = (eng.pair_batch(dP, dQ).cpu().numpy(), eng.multi_pair_fixed_q(P[:48].copy(), Q[:12].copy()), eng.g1_scalar_mul(P, scalars("rel", 64)))
    assert all((a == b).all() for a, b in zip(before, after))


def test_pipelined_small_batches_match_the_two_kernel_form(eng, oracle):
    """Batches of up to 16 384 pairings run the line phase and the accumulator concurrently in one launch
    (k_miller_pipelined: producer blocks publish their line counts, consumer lane pairs wait for them).  Same bytes as the
    two-kernel form (gpbc_set_pipelined_miller(0)) and as the oracle, for sizes around the block edges, with infinities,
    host and device buffers, Miller values and full pairings."""
    import torch
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    g1, g2 = eng.generators()
    n = 16640                                  # one block of 64 beyond the pipelined limit
    P = eng.g1_scalar_mul(g1, scalars("pipe-P", n))
    Q = eng.g2_scalar_mul(g2, scalars("pipe-Q", n))
    P[5] = 0
    Q[64] = 0
    P[n - 1] = 0
    dP, dQ = torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda()
    try:
        _lib.check(lib.gpbc_set_latency_path(0))           # the latency form would take every call of up to 2 048 pairs (it has its own test)
        for m in (1, 2, 31, 32, 33, 63, 64, 65, 1000, 16384, n):
            _lib.check(lib.gpbc_set_pipelined_miller(0))
            f0, e0 = eng.miller_loop(P[:m], Q[:m]), eng.pair_batch(P[:m], Q[:m])
            for mode in (2, 1):                       # 2: no waiting, consumers compute missing lines themselves (the fallback path)
                _lib.check(lib.gpbc_set_pipelined_miller(mode))
                f1, e1 = eng.miller_loop(P[:m], Q[:m]), eng.pair_batch(dP[:m].contiguous(), dQ[:m].contiguous()).cpu().numpy()
                assert (f1 == f0).all() and (e1 == e0).all(), (m, mode)
    finally:
        lib.gpbc_set_pipelined_miller(1)
        lib.gpbc_set_latency_path(2048)
    assert (e1[:200] == oracle.pair_batch(P[:200], Q[:200], threads=8)).all()
    assert e1[5].tobytes() == o.gt_to_bytes(o.F12_ONE) and e1[64].tobytes() == o.gt_to_bytes(o.F12_ONE)


def test_pair_primitives_cross_checked_on_the_device(eng, tmp_path):
    """tools/check_pair_ops.hip: every lane-pair Fp12 primitive (product, squaring, sparse products, both cyclotomic squarings and a run)
    against the single-lane tower, both computed by the same lanes ON the GPU.  The host interval harness proves the arithmetic, but
    it has no DPP: round 3's v_subrev_u32_dpp miscompile (tools/subdpp_probe.hip) passed it and failed here."""
    import shutil
    import subprocess
    from conftest import ROOT
    import os
    exe = os.path.join(ROOT, "tools", "check_pair_ops")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "tools", "check_pair_ops.hip")
    hdrs = [os.path.join(ROOT, "gopairingbasedcryptography_amd", "csrc", f) for f in ("fe29.hip.hpp", "tower29.hip.hpp", "tower29_pair.hip.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in [src] + hdrs):
        exe = str(tmp_path / "check_pair_ops")
        subprocess.check_call([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "gopairingbasedcryptography_amd", "csrc"), src, "-o", exe],
                              stderr=subprocess.DEVNULL, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout and out.stdout.count(" ok ") == 7, out.stdout + out.stderr


def test_latency_path_matches_the_throughput_kernels(eng, oracle):
    """Calls of up to 2 048 pairings take the latency form (csrc/wide29.hip.hpp: one pairing per wavefront, the Miller loop as two waves
    passing lines through an LDS ring, Fp12 values as F2 slots in LDS).  Same bytes as the throughput kernels
    (gpbc_set_latency_path(0)) and as the oracle: Miller values, full pairings, PairingCheck and ragged multi-pairings, sizes around
    the switch-over, points at infinity, host and device buffers."""
    import torch
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    g1, g2 = eng.generators()
    n = 2100
    P = eng.g1_scalar_mul(g1, scalars("wide-P", n))
    Q = eng.g2_scalar_mul(g2, scalars("wide-Q", n))
    P[3] = 0
    Q[70] = 0
    dP, dQ = torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda()
    seg = np.array([0, 2, 2, 5, 9, 10], dtype=np.uint64)
    nP = P[:10].copy(); nP[1] = eng.g1_neg(P[0]); nQ = Q[:10].copy(); nQ[1] = Q[0]        # segment 0: e(P,Q) e(-P,Q) = 1
    try:
        for m in (1, 2, 3, 64, 65, 700, 2048, n):
            _lib.check(lib.gpbc_set_latency_path(0))
            f0, e0 = eng.miller_loop(P[:m], Q[:m]), eng.pair_batch(P[:m], Q[:m])
            _lib.check(lib.gpbc_set_latency_path(2048))
            f1, e1 = eng.miller_loop(P[:m], Q[:m]), eng.pair_batch(dP[:m].contiguous(), dQ[:m].contiguous()).cpu().numpy()
            # Miller values are defined up to factors the final exponentiation removes: compare them through it
            assert (eng.final_exp(f1) == e0).all() and (e1 == e0).all(), m
        for knob in (0, 2048):
            _lib.check(lib.gpbc_set_latency_path(knob))
            mp = eng.multi_pair(nP, nQ, seg)
            ok = eng.pairing_check_batch(nP, nQ, seg)
            assert (mp == oracle.multi_pair(nP, nQ, seg)).all(), knob
            assert list(ok) == [True, True, False, False, False], knob
            # one long segment (the product of 300 Miller values: a serial chain of wide products in the latency form), an empty one, a single
            long_seg = np.array([0, 300, 300, 301], dtype=np.uint64)
            got = eng.multi_pair(P[:301], Q[:301], long_seg)
            if knob == 0:
                want_long = got
            assert (got == want_long).all(), knob
            # segments of 128 values and more on average are folded over 16 wavefronts before the exponentiation (k_segment_fold_wide):
            # lengths below, at and one above the fold, a long one, and a single BSW07-sized segment of 513 pairs
            ragged = np.array([0, 5, 21, 38, 600], dtype=np.uint64)
            got_r, got_1 = eng.multi_pair(P[:600], Q[:600], ragged), eng.multi_pair(P[:513], Q[:513], np.array([0, 513], dtype=np.uint64))
            if knob == 0:
                want_r, want_1 = got_r, got_1
                # the throughput kernels fold long segments too (k_segment_fold: passes of 512 / 64 / 8 lane pairs per segment before
                # the one-thread product) — also over the CHUNK values of the shared-squaring form: 2-pair chunks, 281 of them in one segment
                _lib.check(lib.gpbc_set_multi_pair_chunk(2))
                try:
                    assert (eng.multi_pair(P[:600], Q[:600], ragged) == want_r).all()
                finally:
                    lib.gpbc_set_multi_pair_chunk(0)
            assert (got_r == want_r).all() and (got_1 == want_1).all(), knob
    finally:
        lib.gpbc_set_latency_path(2048)
    assert (e1[:64] == oracle.pair_batch(P[:64], Q[:64], threads=8)).all()
    assert e1[3].tobytes() == o.gt_to_bytes(o.F12_ONE) and e1[70].tobytes() == o.gt_to_bytes(o.F12_ONE)
    assert (want_long == oracle.multi_pair(P[:301], Q[:301], long_seg, threads=8)).all()
    assert (want_r == oracle.multi_pair(P[:600], Q[:600], ragged, threads=8)).all()


def test_multi_pair_fixed_q(eng, oracle, synth):
    """One shared G2 list against k segments of G1 points (precomputed lines): equal to multi_pair on the replicated list
    and to the oracle, for forced chunk lengths and the automatic one; infinities on both sides; device path."""
    import torch
    from gopairingbasedcryptography_amd import _lib
    P, Q = synth
    m, k = 13, 11
    Qs = Q.reshape(-1, 128)[:m].copy()
    Ps = P.reshape(-1, 64)[:m * k].copy()
    Qs[4] = 0                                   # a key component at infinity: skipped by every segment
    Ps[2 * m + 1] = 0
    Ps[5 * m:6 * m] = 0                         # a segment with no finite pair: GT one
    off = np.arange(0, m * k + 1, m).astype(np.uint64)
    want = oracle.multi_pair(Ps, np.tile(Qs, (k, 1)), off, threads=8)
    try:
        for chunk in (8, 3, 1, 0):
            _lib.check(_lib.load().gpbc_set_multi_pair_chunk(chunk))
            assert (eng.multi_pair_fixed_q(Ps, Qs) == want).all(), chunk
            got = eng.multi_pair_fixed_q(torch.from_numpy(Ps).cuda(), torch.from_numpy(Qs).cuda())
            assert (got.cpu().numpy() == want).all(), chunk
    finally:
        _lib.load().gpbc_set_multi_pair_chunk(0)
    assert want[5].tobytes() == o.gt_to_bytes(o.F12_ONE)
    with pytest.raises(ValueError):
        eng.multi_pair_fixed_q(Ps[:m + 1], Qs)
    # long chunks (the BASELINE-size BSW07 decrypt runs 9 chunks of 57): 70 pairs as 64 + 6, 3 x 24 (last one short), 2 x 35
    m, k = 70, 3
    Qs = eng.g2_scalar_mul(Q.reshape(-1, 128)[0], [o.bench_scalar("fq-long-Q", i) for i in range(m)])
    Ps = eng.g1_scalar_mul(P.reshape(-1, 64)[0], [o.bench_scalar("fq-long-P", i) for i in range(m * k)])
    Qs[17] = 0
    Ps[m + 64] = 0                               # a point at infinity inside a group of the batched inversion, in the short chunk
    want = oracle.multi_pair(Ps, np.tile(Qs, (k, 1)), np.arange(0, m * k + 1, m).astype(np.uint64), threads=8)
    try:
        for chunk in (64, 24, 35):
            _lib.check(_lib.load().gpbc_set_multi_pair_chunk(chunk))
            assert (eng.multi_pair_fixed_q(Ps, Qs) == want).all(), chunk
        # the line table of the list: one Q_i per wavefront (k_q_lines_wide, lists within the latency limit) and one per lane
        _lib.check(_lib.load().gpbc_set_latency_path(0))
        assert (eng.multi_pair_fixed_q(Ps, Qs) == want).all()
        _lib.check(_lib.load().gpbc_set_multi_pair_chunk(0))
        assert (eng.multi_pair_fixed_q(Ps, Qs) == want).all()
    finally:
        _lib.load().gpbc_set_multi_pair_chunk(0)
        _lib.load().gpbc_set_latency_path(2048)


def test_bls_verify_flow(eng):
    """signature/bls01_signature/bls_signature_test.go:8-37 shape: sk, pk=[x]g1, sigma=[x]H, PairingCheck."""
    g1, g2 = eng.generators()
    x = o.bench_scalar("bls-sk", 0)
    H = eng.g2_scalar_mul(g2, [o.bench_scalar("bls-H", 0)])[0]      # stand-in for hash-to-G2 (out of scope)
    pk = eng.g1_scalar_mul_base([x])[0]
    sigma = eng.g2_scalar_mul(H, [x])[0]
    neg_sigma = np.frombuffer(o.g2_to_bytes(o.g2_neg(o.g2_from_bytes(sigma.tobytes()))), dtype=np.uint8)
    assert eng.pairing_check(np.concatenate([pk, g1]), np.concatenate([H, neg_sigma]))
    # wrong key / wrong message must fail (bls_signature_test.go:40-72)
    pk_bad = eng.g1_scalar_mul_base([x + 1])[0]
    assert not eng.pairing_check(np.concatenate([pk_bad, g1]), np.concatenate([H, neg_sigma]))
    H_bad = eng.g2_scalar_mul(g2, [o.bench_scalar("bls-H", 1)])[0]
    assert not eng.pairing_check(np.concatenate([pk, g1]), np.concatenate([H_bad, neg_sigma]))


def test_zss_signature_identity(eng):
    """The ZSS verification equation of the reference (signature/zss04_signature/zss04_signature.go:321-341):
    sigma = [1 / (H(m) + x)] g1, pk = [x] g2, and e(sigma, [H(m)] g2 + pk) must equal e(g1, g2) — for a batch of messages,
    with the G2 addition done by the engine's point-sum kernel; a signature under another key must fail."""
    n = 48
    g1, g2 = eng.generators()
    x = o.bench_scalar("zss-x", 0)
    hs = [o.bench_scalar("zss-h", i) for i in range(n)]
    inv = [pow((h + x) % o.R, -1, o.R) for h in hs]
    sigma = eng.g1_scalar_mul(g1, inv)
    pk = eng.g2_scalar_mul(g2, [x])[0]
    hg2 = eng.g2_scalar_mul(g2, hs)
    rhs_pts = np.stack([eng.g2_sum(np.concatenate([hg2[i], pk])) for i in range(n)]).reshape(n, 128)
    lhs = eng.pair_batch(sigma, rhs_pts)
    e = eng.pair(g1, g2)
    assert all((lhs[i] == e).all() for i in range(n))
    other = eng.g2_scalar_mul(g2, [x + 1])[0]
    bad = eng.pair_batch(sigma[:4], np.stack([eng.g2_sum(np.concatenate([hg2[i], other])) for i in range(4)]).reshape(4, 128))
    assert not any((bad[i] == e).all() for i in range(4))


def test_scalar_mul_golden(eng):
    for name, fn in (("g1_scalar_mul.json", eng.g1_scalar_mul), ("g2_scalar_mul.json", eng.g2_scalar_mul)):
        g = load_golden(name)["cases"]
        out = fn(cat([c["base"] for c in g]), cat([c["scalar"] for c in g]))
        for i, c in enumerate(g):
            assert out[i].tobytes().hex() == c["out"], (name, i, c["note"])


def test_scalar_mul_vs_oracle(eng, oracle, synth):
    P, Q = synth
    n = P.shape[0]
    k = scalars("s", n)
    assert (eng.g1_scalar_mul(P, k) == oracle.g1_scalar_mul(P, k, threads=8)).all()
    assert (eng.g2_scalar_mul(Q, k) == oracle.g2_scalar_mul(Q, k, threads=8)).all()
    # shared base == per-element base
    assert (eng.g1_scalar_mul(P[0], k) == eng.g1_scalar_mul(np.tile(P[0], n), k)).all()


def test_point_sums(eng, oracle, synth):
    P, Q = synth
    for n in (1, 2, 31, 32, 33, 192):
        assert (eng.g1_sum(P[:n]) == oracle.g1_sum(P[:n])).all(), n
        assert (eng.g2_sum(Q[:n]) == oracle.g2_sum(Q[:n])).all(), n
    # P + (-P) + inf -> inf
    neg = np.frombuffer(o.g1_to_bytes(o.g1_neg(o.g1_from_bytes(P[0].tobytes()))), dtype=np.uint8)
    assert not eng.g1_sum(np.concatenate([P[0], neg, np.zeros(64, dtype=np.uint8)])).any()
    assert not eng.g1_sum(np.zeros(0, dtype=np.uint8)).any()


def test_scalar_mul_one_point_per_quad_and_per_lane_agree(eng, oracle):
    """Calls of up to 2 048 G2 points run one point per OCTET of lanes, calls of up to 16 384 points one point per QUAD of lanes (csrc/curve29_quad.hip.hpp: the loop's doublings and additions three
    products wide), larger ones one point per lane: the same random points and 256-bit scalars through both, and against the oracle on a
    sample; infinity, zero and tiny scalars, and a shared base included."""
    g1, g2 = eng.generators()
    n = 16385
    rng = np.random.default_rng(77)
    k1 = rng.integers(0, 256, size=(n, 32), dtype=np.uint8); k1[:, 31] &= 0x1f
    k2 = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    k2[:4] = 0; k2[1, 0], k2[2, 0], k2[3, 0] = 1, 2, 3
    pick = np.r_[0:8, 100:108, n - 9:n - 1]
    for gen, mul, omul, w in ((g1, eng.g1_scalar_mul, oracle.g1_scalar_mul, 64), (g2, eng.g2_scalar_mul, oracle.g2_scalar_mul, 128)):
        base = mul(gen, k1.reshape(-1)).reshape(n, w).copy()       # n > 16 384 with one shared base: the fixed-base path
        base[5] = 0
        lane = mul(base, k2.reshape(-1)).reshape(n, w)              # one point per lane
        quad = mul(base[:16384], k2[:16384].reshape(-1)).reshape(16384, w)
        assert (quad == lane[:16384]).all()
        # calls of up to 2 048 points: G2 runs one point per OCTET of lanes (csrc/curve29_oct.hip.hpp: half Fp2 products on lane pairs)
        for lo, hi in ((0, 2048), (0, 1), (5, 6), (100, 107), (3000, 5047)):
            assert (mul(base[lo:hi], k2[lo:hi].reshape(-1)).reshape(hi - lo, w) == lane[lo:hi]).all(), (w, lo, hi)
        assert (lane[pick] == np.asarray(omul(base[pick], k2[pick].reshape(-1), threads=8)).reshape(-1, w)).all()
        if w == 128:                                                # G2 decoding: the subgroup test per quad (<= 16 384) and per lane
            enc = np.asarray(eng.g2_marshal(lane, compressed=True)).reshape(n, 64)
            back_l, ok_l = eng.g2_unmarshal(enc.reshape(-1), elem_bytes=64)
            back_q, ok_q = eng.g2_unmarshal(enc[:16384].reshape(-1), elem_bytes=64)
            assert ok_l.all() and ok_q.all() and (back_l == lane).all() and (back_q == lane[:16384]).all()
            bad = enc.copy(); bad[9, 40] ^= 1; bad[16384, 40] ^= 1    # a flipped bit of x: no square root, or a point outside the subgroup
            _, okb_l = eng.g2_unmarshal(bad.reshape(-1), elem_bytes=64)
            _, okb_q = eng.g2_unmarshal(bad[:16384].reshape(-1), elem_bytes=64)
            assert not okb_l[9] and not okb_l[16384] and not okb_q[9] and okb_l.sum() == n - 2 and okb_q.sum() == 16383
            back_o, ok_o = eng.g2_unmarshal(enc[:2048].reshape(-1), elem_bytes=64)                 # ... and per octet (<= 2 048)
            _, okb_o = eng.g2_unmarshal(bad[:2048].reshape(-1), elem_bytes=64)
            assert ok_o.all() and (back_o == lane[:2048]).all() and not okb_o[9] and okb_o.sum() == 2047
            m2, ok2 = eng.g2_unmarshal(np.asarray(eng.g2_marshal(lane[:2048], compressed=False)).reshape(-1), elem_bytes=128)   # raw form
            assert ok2.all() and (m2 == lane[:2048]).all()
        shared = mul(base[7], k2[:300].reshape(-1)).reshape(300, w)  # one base, 300 scalars: the quad kernel's shared-base form
        assert (shared == np.asarray(omul(np.tile(base[7], (300, 1)), k2[:300].reshape(-1), threads=8)).reshape(-1, w)).all()


def test_scalar_mul_base_through_generator_tables(eng, oracle):
    """ScalarMultiplicationBase for small host calls runs on fixed-base tables of the generators (as the C++ and Go host sides do):
    same bytes as the variable-base kernel on the generator and as the oracle, zero and r - 1 and a 256-bit pattern included."""
    g1, g2 = eng.generators()
    ks = [0, 1, 2, o.R - 1] + [o.bench_scalar("base", i) for i in range(28)]
    kb = eng.scalars_to_bytes(ks)
    for base, mul_base, mul, omul in ((g1, eng.g1_scalar_mul_base, eng.g1_scalar_mul, oracle.g1_scalar_mul), (g2, eng.g2_scalar_mul_base, eng.g2_scalar_mul, oracle.g2_scalar_mul)):
        got = mul_base(ks)
        assert (got == mul(base, kb)).all() and (np.asarray(got).reshape(-1) == np.asarray(omul(base, kb)).reshape(-1)).all()
        assert (mul_base([ks[5]]) == got[5:6]).all()


def test_gt_ops_golden(eng):
    g = load_golden("gt_ops.json")
    out = eng.gt_exp(cat([c["x"] for c in g["exp"]]), cat([c["k"] for c in g["exp"]]))
    for i, c in enumerate(g["exp"]):
        assert out[i].tobytes().hex() == c["out"], i
    a, b = cat([c["a"] for c in g["binary"]]), cat([c["b"] for c in g["binary"]])
    mul, div, inv = eng.gt_mul(a, b), eng.gt_div(a, b), eng.gt_inverse(a)
    for i, c in enumerate(g["binary"]):
        assert mul[i].tobytes().hex() == c["mul"]
        assert div[i].tobytes().hex() == c["div"]
        assert inv[i].tobytes().hex() == c["inv_a"]
    # negative exponent = inverse then exp (gnark GT.Exp)
    x = hx(g["exp"][5]["x"])
    assert (eng.gt_exp(x, [-7]) == eng.gt_exp(eng.gt_inverse(x), [7])).all()


def test_gt_exp_vs_oracle(eng, oracle, synth):
    """GT.Exp through both forms — one element per lane pair (gpbc_set_latency_path(0)) and one per wavefront (calls of up to 2 048
    elements, wide_exp256) — on pairing values and on Miller values (Fp12 elements OUTSIDE the cyclotomic subgroup: gnark's Exp is the
    generic square-and-multiply), with the edge exponents 0, 1, 2, 7, 8, r - 1, r, 2^255 and 2^256 - 1 among random ones."""
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    P, Q = synth[0][:40], synth[1][:40]
    gt = eng.pair_batch(P, Q)
    gt[20:] = eng.miller_loop(P[20:], Q[20:])
    gt[19] = 0                                                 # the zero element: 0^k = 0, 0^0 = 1 (it passes the subgroup test: 0 * 0 == 0)
    k = scalars("gtexp", 40).reshape(40, 32).copy()
    for i, e in enumerate((0, 1, 2, 7, 8, o.R - 1, o.R, 1 << 255, (1 << 256) - 1)):
        k[i] = k[20 + i] = np.frombuffer(e.to_bytes(32, "little"), dtype=np.uint8)
    want = oracle.gt_exp(gt, k.reshape(-1), threads=8)
    # wavefronts (32 elements) of pairing values only square by Granger-Scott, any other element in a wavefront sends it down the
    # general path: `gt` mixes both in its first wavefront, `gt_c` is cyclotomic throughout
    gt_c = eng.pair_batch(P, Q)
    want_c = oracle.gt_exp(gt_c, k.reshape(-1), threads=8)
    try:
        for knob in (0, 2048):
            _lib.check(lib.gpbc_set_latency_path(knob))
            assert (eng.gt_exp(gt, k.reshape(-1)) == want).all(), knob
            assert (eng.gt_exp(gt_c, k.reshape(-1)) == want_c).all(), knob
            assert (eng.gt_exp(gt[:1], k[:1].reshape(-1)) == want[:1]).all() and (eng.gt_exp(gt[3:4], k[3:4].reshape(-1)) == want[3:4]).all(), knob
    finally:
        lib.gpbc_set_latency_path(2048)


def test_gt_div_and_inverse_on_any_divisor(eng, oracle, synth):
    """GT.Div / GT.Inverse take the conjugate when every divisor of a wavefront has norm one (pairing values) and the Fp6 inversion
    otherwise: wavefronts (64 elements) of pairing values only, of Miller values only (norm not one), and mixed — against the oracle."""
    P, Q = synth[0][:160], synth[1][:160]
    a = eng.pair_batch(P, Q)
    b = eng.pair_batch(P[::-1].copy(), Q)
    b[64:128] = eng.miller_loop(P[64:128], Q[64:128])          # second wavefront: general divisors
    b[130:140] = eng.miller_loop(P[130:140], Q[130:140])       # third: mixed
    b[141] = 0                                                 # 1 / 0 = 0 (gnark's Inverse convention, the oracle's too)
    assert (eng.gt_div(a, b) == oracle.gt_div(a, b)).all()
    assert (eng.gt_inverse(b) == oracle.gt_inverse(b)).all()
    assert (eng.gt_div(a[:1], b[:1]) == oracle.gt_div(a[:1], b[:1])).all() and (eng.gt_inverse(b[64:65]) == oracle.gt_inverse(b[64:65])).all()


def test_bilinearity_property(eng, synth):
    """e([a]P,[b]Q) == e(P,Q)^(ab) and the restructuring identities of SURVEY §8a-3, all on the GPU."""
    P, Q = synth[0][:16], synth[1][:16]
    a = [o.bench_scalar("bil-a", i) for i in range(16)]
    b = [o.bench_scalar("bil-b", i) for i in range(16)]
    lhs = eng.pair_batch(eng.g1_scalar_mul(P, a), eng.g2_scalar_mul(Q, b))
    rhs = eng.gt_exp(eng.pair_batch(P, Q), [x * y % o.R for x, y in zip(a, b)])
    assert (lhs == rhs).all()
    # product of 16 pairings with one final exponentiation == product of 16 full pairings
    one_fe = eng.multi_pair(P, Q, [0, 16])[0]
    full = eng.pair_batch(P, Q)
    acc = full[0]
    for i in range(1, 16):
        acc = eng.gt_mul(acc, full[i])[0]
    assert (one_fe == acc).all()


def test_device_pointer_path(eng, synth):
    """HBM-resident buffers through the *_dev entry points on torch's current stream."""
    import torch
    P, Q = synth
    dP = torch.from_numpy(np.ascontiguousarray(P)).cuda()
    dQ = torch.from_numpy(np.ascontiguousarray(Q)).cuda()
    host = eng.pair_batch(P, Q)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = eng.pair_batch(dP, dQ)
        mp = eng.multi_pair(dP, dQ, np.array([0, 5, 5, 192]))
    s.synchronize()
    assert (dev.cpu().numpy() == host).all()
    assert (mp.cpu().numpy() == eng.multi_pair(P, Q, [0, 5, 5, 192])).all()
    k = torch.from_numpy(scalars("s", P.shape[0]).copy()).cuda()
    assert (eng.g1_scalar_mul(dP, k).cpu().numpy() == eng.g1_scalar_mul(P, k.cpu().numpy())).all()
    assert (eng.g1_sum(dP).cpu().numpy() == eng.g1_sum(P)).all()
    with pytest.raises(ValueError, match="invalid inputs sizes"):       # segment table must cover exactly the pairs given
        eng.multi_pair(dP, dQ, np.array([0, 5, 500]))
    with pytest.raises(ValueError, match="invalid inputs sizes"):
        eng.multi_pair(P, Q, np.array([0, 5, 100]))
    # a segment table that lives in device memory is validated on the device (gpbc_check_segments_dev) before it is used
    dseg = lambda v: torch.tensor(v, dtype=torch.int64).cuda()
    assert (eng.multi_pair(dP, dQ, dseg([0, 5, 5, 192])).cpu().numpy() == eng.multi_pair(P, Q, [0, 5, 5, 192])).all()
    for bad in ([0, 9, 5, 192], [1, 5, 192], [0, 5, 191], [0, 5, 1 << 40]):
        with pytest.raises(ValueError, match="invalid inputs sizes"):
            eng.multi_pair(dP, dQ, dseg(bad))


def test_cpp_host_mirror_bls_flow(eng, tmp_path):
    """include/gpbc_bn254.hpp (C++ mirror of the gnark surface) running the reference's BLS test flow on the GPU."""
    import subprocess
    from conftest import ROOT
    import os
    exe = str(tmp_path / "test_bls_flow")
    pkg = os.path.join(ROOT, "gopairingbasedcryptography_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_bls_flow.cpp"),
                           "-L" + pkg, "-lgpbc_bn254", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "BLS flow OK" in out.stdout, out.stdout + out.stderr


def test_concurrent_host_threads(eng, tmp_path):
    """Six host threads on the host-pointer API at once (shared default stream and internal workspace): every thread
    gets a lone caller's results."""
    import subprocess
    from conftest import ROOT
    import os
    exe = str(tmp_path / "test_threads")
    pkg = os.path.join(ROOT, "gopairingbasedcryptography_amd")
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_threads.cpp"),
                           "-L" + pkg, "-lgpbc_bn254", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "threads OK" in out.stdout, out.stdout + out.stderr


def test_one_process_drives_every_device(eng, tmp_path):
    """tests/cpp/test_multi_device.cpp: ONE process binds every visible GPU through the C ABI (gpbc_init_devices): sharded
    host-pointer entries must return one device's bits, one thread per device runs *_dev entries, the RCCL all-gather runs
    inside the library, and BLS aggregate verification goes through gpbc_g1/g2_scalar_mul_sum.  With one GPU the list is
    {0, 0} (two slots share it) so the sharding code still runs."""
    import subprocess
    from conftest import ROOT
    import os
    exe = str(tmp_path / "test_multi_device")
    pkg = os.path.join(ROOT, "gopairingbasedcryptography_amd")
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-w", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_multi_device.cpp"),
                           "-L" + pkg, "-lgpbc_bn254", "-Wl,-rpath," + pkg, "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "multi-device OK" in out.stdout, out.stdout + out.stderr


def _multi_device_on_the_test_double(tmp_path, slots):
    import subprocess
    from conftest import ROOT
    import os
    stub_dir = str(tmp_path / "stub_rccl")
    os.makedirs(stub_dir)
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", "-pthread", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "stub_rccl", "rccl_stub.cpp"), "-L/opt/rocm/lib", "-lamdhip64", "-o", os.path.join(stub_dir, "librccl.so.1")])
    exe = str(tmp_path / "test_multi_device")
    pkg = os.path.join(ROOT, "gopairingbasedcryptography_amd")
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-w", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_multi_device.cpp"),
                           "-L" + pkg, "-lgpbc_bn254", "-Wl,-rpath," + pkg, "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
    env = dict(os.environ, GPBC_TEST_STUB_RCCL="1", GPBC_TEST_SLOTS=str(slots), LD_LIBRARY_PATH=stub_dir + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=1100, env=env)
    assert out.returncode == 0 and "multi-device OK" in out.stdout, out.stdout + out.stderr
    assert "%d bound slot(s)" % slots in out.stdout, out.stdout
    assert "RCCL all-gather over %d rank(s) inside the library (rccl TEST DOUBLE" % slots in out.stdout, out.stdout
    assert "scalar_mul_sum_dev on %d rank(s)" % slots in out.stdout and "BLS aggregate verify over %d rank(s)" % slots in out.stdout, out.stdout


def test_collective_paths_with_eight_ranks_on_a_test_double(eng, tmp_path):
    """The rank arithmetic of BASELINE's 8-GPU node, rehearsed in ONE process on this one GPU: tests/cpp/test_multi_device.cpp with
    the device listed eight times (GPBC_TEST_SLOTS=8) over tests/stub_rccl — host entries sharded over 8 slots with ragged shares
    (34 002 units: 4 251 and 4 250 per slot), one host thread per slot on *_dev entries, ncclCommInitAll over 8 ranks, rank order and
    offsets of the gathered GT rows on every rank (config 5's shape: n/G x 384 B), scalar_mul_sum_dev with the 64 / 128-byte
    partial sums all-gathered (config 3's shape: 192 B per rank) on every rank, aggregate verification accept / reject.  One process
    because the pool allows six GPU processes at a time; the multi-PROCESS form runs with four ranks below.  Test infrastructure
    only: real RCCL with more than one rank has never run here and multi-GPU rates remain UNMEASURED ON HARDWARE."""
    _multi_device_on_the_test_double(tmp_path, 8)


def test_collective_paths_with_two_ranks_on_a_test_double(eng, tmp_path):
    """The N > 1 collective code of the library — ncclCommInitAll over two slots, the grouped ncclAllGather of
    gpbc_allgather_all_dev (rank order, offsets), the per-rank ncclAllGather inside gpbc_g1/g2_scalar_mul_sum_dev, a 10 000-signature
    aggregate verification with a forged-signature reject on the gathered sums — executed with TWO ranks on the one GPU of this box:
    real RCCL refuses the device list {0, 0}, so tests/stub_rccl/rccl_stub.cpp (a ~150-line librccl.so.1 that rendezvouses the
    ranks on the host and copies device to device) stands in for it, found through LD_LIBRARY_PATH by the library's dlopen.  Test
    infrastructure only: the product keeps real RCCL, and multi-GPU RATES remain unmeasured on hardware."""
    _multi_device_on_the_test_double(tmp_path, 2)


def test_two_process_ranks_over_the_test_double(eng, tmp_path):
    """bench.py --gpus 2 as the driver launches it (torch.distributed.run, one process per rank), rehearsed on this one GPU with the
    library communicator over tests/stub_rccl (GPBC_BENCH_REHEARSAL=stub, GPBC_RCCL_LIBRARY): gpbc_comm_get_unique_id ->
    gpbc_comm_init_rank with TWO ranks -> gpbc_allgather_dev / gpbc_g1_scalar_mul_sum_dev inside the three strong-scaling legs
    (aggregate verification, BSW07 decrypt, AFP25 decrypt + all-gather of the GT masks), each checked by the bench itself.  Not a
    measurement — it shows the N > 1 code of the C library and of bench.py runs and returns right answers."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    import os
    stub = str(tmp_path / "librccl.so.1")
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", "-pthread", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "stub_rccl", "rccl_stub.cpp"), "-L/opt/rocm/lib", "-lamdhip64", "-lrt", "-o", stub])
    env = dict(os.environ, GPBC_BENCH_REHEARSAL="stub", GPBC_RCCL_LIBRARY=stub, HSA_ENABLE_IPC_MODE_LEGACY="0")
    # two ranks at even sizes, then FOUR ranks with ragged ones (--batch 16387; --config-scale 61: 17 189 signatures = 4 298 + 3 x 4 297,
    # 1 074 ciphertexts = 269 + 269 + 268 + 268).  Four, not eight, rank processes: the pool allows six GPU processes at a time and the
    # test runner is one of them; the 8-rank arithmetic runs in one process above.
    for ranks, batch, scale, port in ((2, "16384", "64", "29531"), (4, "16387", "61", "29533")):
        out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1", "--master-port", port,
                              os.path.join(ROOT, "bench.py"), "--gpus", str(ranks), "--steps", "1", "--warmup", "1", "--batch", batch, "--config-scale", scale, "--full", "--no-cpu"],
                             capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        line = json.loads(out.stdout.strip().splitlines()[-1])
        assert line["n_gpus"] == ranks and "TEST DOUBLE" in line["config"]["rehearsal"]
        legs = line["secondary"]["configs"]
        assert legs.get("comm_error") is None, legs
        for name in ("aggregate_verify_2^20", "bsw07_256of256_2^16", "afp25_2^18"):
            assert "error" not in legs[name], (ranks, name, legs[name])
        assert legs["aggregate_verify_2^20"]["accepts"] and legs["aggregate_verify_2^20"]["rejects_forged"]
        assert legs["bsw07_256of256_2^16"]["all_messages_recovered"]
        assert legs["afp25_2^18"]["all_messages_recovered"] and legs["afp25_2^18"]["collective"]
        assert ("%d ranks" % ranks) in legs["aggregate_verify_2^20"]["collective"]


def test_large_batch_chunks_and_properties(eng, oracle):
    """BASELINE size (2^20 would take the oracle ~1 min on one core, so 2^18 + 5 pairs here: more than one lines-workspace
    chunk of 262144, ragged tail): HBM-resident path, spot-checked against the oracle at chunk boundaries, plus
    size-independent properties over the whole batch: e(P,Q)*e(-P,Q) == 1 per element through multi_pair, and
    e([2]P,Q) == e(P,Q)^2 as a checksum of all outputs."""
    import torch
    n = (1 << 18) + 5
    g1, g2 = eng.generators()
    rng = np.random.default_rng(20)
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint8).copy().reshape(n, 32)
    k[:, 31] &= 0x1F                                            # < 2^253 < r
    dk = torch.from_numpy(k).cuda()
    dP = eng.g1_scalar_mul(torch.from_numpy(g1).cuda(), dk)
    dQ = eng.g2_scalar_mul(torch.from_numpy(g2).cuda(), dk.flip(0).contiguous())
    gt = eng.pair_batch(dP, dQ)
    torch.cuda.synchronize()
    idx = np.array([0, 1, 63, 64, 262143, 262144, 262145, n - 2, n - 1, 131071, 200000])
    P, Q, G = dP[idx].cpu().numpy(), dQ[idx].cpu().numpy(), gt[idx].cpu().numpy()
    assert (G == oracle.pair_batch(P, Q, threads=8)).all()
    # e([2]P, Q) == e(P,Q)^2 for every element (GPU-only identity over the full batch)
    two = torch.from_numpy(np.tile(np.frombuffer((2).to_bytes(32, "little"), dtype=np.uint8), n).reshape(n, 32).copy()).cuda()
    gt2 = eng.pair_batch(eng.g1_scalar_mul(dP, two), dQ)
    sq = eng.gt_mul(gt, gt)
    assert bool((gt2 == sq).all())
    # product with the negated point is one: multi_pair with 2-pair segments
    m = 4096
    negP = dP[:m].cpu().numpy().copy()
    for i in range(m):
        negP[i] = np.frombuffer(o.g1_to_bytes(o.g1_neg(o.g1_from_bytes(negP[i].tobytes()))), dtype=np.uint8)
    PP = np.stack([dP[:m].cpu().numpy(), negP], axis=1).reshape(-1, 64)
    QQ = np.repeat(dQ[:m].cpu().numpy(), 2, axis=0)
    ok = eng.pairing_check_batch(PP, QQ, np.arange(0, 2 * m + 1, 2))
    assert ok.all()


def test_multi_pair_cpabe_shape(eng, oracle):
    """BASELINE config 4 shape at test size: 513-pair products (256-attribute BSW07 decrypt: 2*256+1 pairs),
    16 ciphertexts, one final exponentiation per segment, against the oracle."""
    import torch
    segs, m = 16, 513
    n = segs * m
    g1, g2 = eng.generators()
    rng = np.random.default_rng(513)
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint8).copy().reshape(n, 32)
    k[:, 31] &= 0x1F
    dk = torch.from_numpy(k).cuda()
    P = eng.g1_scalar_mul(torch.from_numpy(g1).cuda(), dk).cpu().numpy()
    Q = eng.g2_scalar_mul(torch.from_numpy(g2).cuda(), dk.flip(0).contiguous()).cpu().numpy()
    off = np.arange(0, n + 1, m)
    assert (eng.multi_pair(P, Q, off) == oracle.multi_pair(P, Q, off, threads=16)).all()


def test_aggregate_verify_single_gpu(eng):
    """BASELINE config 3 shape on one GPU (world size 1, no process group): 4096 BLS signatures on one message point,
    random-linear-combination aggregate check through sharding.aggregate_verify with the real engine; one forged
    signature must make it fail."""
    import torch
    from gopairingbasedcryptography_amd import sharding
    n = 4096
    g1, g2 = eng.generators()
    rng = np.random.default_rng(3)
    x = np.frombuffer(rng.bytes(32 * n), dtype=np.uint8).copy().reshape(n, 32); x[:, 31] &= 0x1F
    rho = np.frombuffer(rng.bytes(32 * n), dtype=np.uint8).copy().reshape(n, 32); rho[:, 16:] = 0
    H = eng.g2_scalar_mul(g2, [o.bench_scalar("H", 0)])[0]
    pk = eng.g1_scalar_mul(g1, x)
    sig = eng.g2_scalar_mul(H, x)
    neg = lambda b: np.frombuffer(o.g2_to_bytes(o.g2_neg(o.g2_from_bytes(np.asarray(b, dtype=np.uint8).tobytes()))), dtype=np.uint8)
    assert sharding.aggregate_verify(eng, pk, rho, sig, H, g1, neg) is True
    sig2 = sig.copy(); sig2[n // 2] = eng.g2_scalar_mul(H, [12345])[0]
    assert sharding.aggregate_verify(eng, pk, rho, sig2, H, g1, neg) is False
    # HBM-resident inputs take the same path
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert sharding.aggregate_verify(eng, d(pk), d(rho), d(sig), H, g1, neg) is True


def test_bsw07_batched_decrypt_on_gpu(eng, oracle):
    """Config 4 semantics on the GPU engine: keys, ciphertexts, folded one-multi-pairing decryption of 6 ciphertexts; the
    result equals the message and the oracle's reference-shaped (pairing-by-pairing) evaluation bit for bit."""
    from bsw07_fixture import Instance, example_tree
    from gopairingbasedcryptography_amd import bsw07
    inst = Instance(eng, example_tree(), user_attrs=[11, 22, 33], n_ct=6)
    plan = bsw07.decrypt_plan(inst.tree, inst.user_attrs)
    folded = bsw07.fold_key(eng, plan, inst.dj, inst.dj_prime)
    out = bsw07.decrypt_batch(eng, folded, inst.D, inst.cts, Instance.neg_g1)
    for t, ct in enumerate(inst.cts):
        assert (out[t] == inst.msgs[t]).all()
        assert (out[t] == inst.reference_shaped_decrypt(oracle, ct)).all()


def test_afp25_batched_decrypt_on_gpu(eng, oracle):
    """Config 5 semantics on the GPU engine: batch of 8 identities, 5 ciphertexts decrypted with one multi_pair call."""
    from afp25_fixture import Instance
    from gopairingbasedcryptography_amd import afp25
    inst = Instance(eng, B=8, n_items=5)
    out = afp25.decrypt_batch(eng, inst.g1, inst.tau_powers, inst.D, inst.f, inst.sk, inst.items)
    for t, item in enumerate(inst.items):
        assert (out[t] == inst.msgs[t]).all()
        assert (out[t] == inst.reference_shaped_decrypt(oracle, item)).all()


def test_fixed_base_msm(eng, oracle, synth):
    """Fixed-base window tables: single base (ScalarMultiplicationBase) against the oracle with edge scalars, several
    bases against the variable-base kernels + point sums, G1 and G2, host and device paths, a base at infinity."""
    import torch
    g1, g2 = eng.generators()
    P, Q = synth
    edge = [0, 1, 2, 255, 256, o.R - 1, o.R, o.R + 1, (1 << 256) - 1, 1 << 255] + [o.bench_scalar("fb", i) for i in range(54)]
    kb = np.frombuffer(b"".join((k % (1 << 256)).to_bytes(32, "little") for k in edge), dtype=np.uint8)
    fb1 = eng.FixedBase(g1)
    assert fb1.table_bytes() == 32 * 255 * 128
    assert (fb1.mul(kb) == oracle.g1_scalar_mul(g1, kb, threads=8)).all()
    fb2 = eng.FixedBase(g2, g2=True)
    assert (fb2.mul(kb) == oracle.g2_scalar_mul(g2, kb, threads=8)).all()
    # multi-base: 37 bases (one at infinity), 19 sums
    nb, nm = 37, 19
    for pts, is_g2, smul, psum, w in ((P, False, eng.g1_scalar_mul, eng.g1_sum, 64), (Q, True, eng.g2_scalar_mul, eng.g2_sum, 128)):
        bases = np.ascontiguousarray(pts[:nb]).copy()
        bases[5] = 0
        ks = scalars("fbm", nb * nm).reshape(nm, nb * 32)
        fb = eng.FixedBase(bases, g2=is_g2)
        got = fb.msm(ks)
        for m in range(nm):
            want = psum(smul(bases, ks[m]))
            assert (got[m] == np.asarray(want).reshape(-1)).all(), (is_g2, m)
        got_dev = fb.msm(torch.from_numpy(ks.copy()).cuda())
        assert (got_dev.cpu().numpy() == got).all()
        fb.close()
    # large single-base batch through the device path (more lanes than one launch wave): every row equals the variable-base kernel
    n = 1 << 15
    kd = torch.from_numpy(scalars("fbl", n).copy()).cuda()
    g1d, g2d = torch.from_numpy(g1).cuda(), torch.from_numpy(g2).cuda()
    general = eng.g1_scalar_mul(g1d.repeat(n), kd)                      # one base per scalar: the variable-base kernel
    assert torch.equal(fb1.mul(kd), general)
    # a shared base with n >= 16384 goes through a transient table inside gpbc_g1/g2_scalar_mul_batch itself
    assert torch.equal(eng.g1_scalar_mul(g1d, kd), general)
    assert torch.equal(eng.g2_scalar_mul(g2d, kd), eng.g2_scalar_mul(g2d.repeat(n), kd))
    zero_base = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert not bool(eng.g1_scalar_mul(zero_base, kd).any())             # [k] infinity = infinity


def test_scalar_mul_chunked_batch_against_fixed_base(eng):
    """More points than one table-workspace chunk (262 144) through the variable-base kernel, checked row by row against
    an independent kernel: [k_i]([a_i] g1) must equal [k_i a_i mod r] g1 from the fixed-base table path."""
    import torch
    n = (1 << 18) + 7
    g1, _ = eng.generators()
    a = [o.bench_scalar("ca", i) for i in range(n)]
    k = [o.bench_scalar("ck", i) for i in range(n)]
    to_dev = lambda xs: torch.from_numpy(np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype=np.uint8).copy()).cuda()
    fb = eng.FixedBase(g1)
    bases = fb.mul(to_dev(a))                                            # [n, 64] distinct bases
    got = eng.g1_scalar_mul(bases, to_dev(k))                            # nbase == n: chunked variable-base launches
    want = fb.mul(to_dev([x * y % o.R for x, y in zip(a, k)]))
    assert torch.equal(got, want)


def test_afp25_openings_by_fixed_base_msm(eng, oracle):
    """AFP25 batch decryption with the opening proofs from ONE fixed-base MSM over the SRS (afp25.srs_table): same
    messages, same bits as the per-item path."""
    from afp25_fixture import Instance
    from gopairingbasedcryptography_amd import afp25
    inst = Instance(eng, B=8, n_items=5)
    table = afp25.srs_table(eng, inst.g1, inst.tau_powers)
    a = afp25.decrypt_batch(eng, inst.g1, inst.tau_powers, inst.D, inst.f, inst.sk, inst.items, table=table)
    b = afp25.decrypt_batch(eng, inst.g1, inst.tau_powers, inst.D, inst.f, inst.sk, inst.items)
    assert (np.asarray(a) == np.asarray(b)).all()
    for t in range(len(inst.items)):
        assert (a[t] == inst.msgs[t]).all()


# ---------------------------------------------------------------------------------------- wire formats (§8 f-4)
def test_wire_golden(eng):
    g = load_golden("wire.json")
    for key, marshal, unmarshal in (("g1", eng.g1_marshal, eng.g1_unmarshal), ("g2", eng.g2_marshal, eng.g2_unmarshal)):
        cs = g[key]
        mem = cat([c["mem"] for c in cs])
        for comp, field in ((False, "raw"), (True, "compressed")):
            enc = marshal(mem, compressed=comp)
            for i, c in enumerate(cs):
                assert enc[i].tobytes().hex() == c[field], (key, field, c["note"])
            dec, ok = unmarshal(cat([c[field] for c in cs]), elem_bytes=enc.shape[1])
            assert ok.all() and dec.tobytes() == mem.tobytes(), (key, field)
        for c in g["decode_" + key]:
            dec, ok = unmarshal(hx(c["wire"]), elem_bytes=c["elem_bytes"])
            assert int(ok[0]) == c["ok"] and dec[0].tobytes().hex() == c["mem"], (key, c["note"])
    cs = g["gt"]
    mem = cat([c["mem"] for c in cs])
    assert eng.gt_marshal(mem).tobytes().hex() == "".join(c["wire"] for c in cs)
    dec, ok = eng.gt_unmarshal(cat([c["wire"] for c in cs]))
    assert ok.all() and dec.tobytes() == mem.tobytes()
    for c in g["decode_gt"]:
        dec, ok = eng.gt_unmarshal(hx(c["wire"]))
        assert int(ok[0]) == c["ok"] and dec[0].tobytes().hex() == c["mem"], c["note"]
    with pytest.raises(ValueError):
        eng.g1_unmarshal(np.zeros(48, dtype=np.uint8), elem_bytes=48)


def test_wire_vs_oracle_and_corruption(eng, synth):
    """Engine encodings of the synthetic points against the big-integer oracle, then bit flips: the engine and the oracle
    must accept / reject the same buffers and agree on every accepted point."""
    P, Q = synth
    n = 24
    rng = np.random.default_rng(99)
    for pts, w, marshal, unmarshal, from_mem, to_mem, o_marshal, o_unmarshal in (
            (P, 64, eng.g1_marshal, eng.g1_unmarshal, o.g1_from_bytes, o.g1_to_bytes, o.g1_marshal, o.g1_unmarshal),
            (Q, 128, eng.g2_marshal, eng.g2_unmarshal, o.g2_from_bytes, o.g2_to_bytes, o.g2_marshal, o.g2_unmarshal)):
        pts = np.ascontiguousarray(pts[:n])
        for comp in (False, True):
            enc = marshal(pts, compressed=comp)
            for i in range(n):
                assert enc[i].tobytes() == o_marshal(from_mem(pts[i].tobytes()), comp), (w, comp, i)
            bad = enc.copy()
            for i in range(n):
                for _ in range(int(rng.integers(1, 3))):
                    bad[i, int(rng.integers(0, bad.shape[1]))] ^= np.uint8(1 << int(rng.integers(0, 8)))
            dec, ok = unmarshal(bad, elem_bytes=bad.shape[1])
            for i in range(n):
                pt, good = o_unmarshal(bad[i].tobytes())
                assert int(good) == int(ok[i]), (w, comp, i)
                assert dec[i].tobytes() == to_mem(pt if good else None), (w, comp, i)


def test_wire_round_trip_large_device_path(eng):
    """Size-independent property at a large batch, HBM-resident: unmarshal(marshal(X)) == X with every ok flag set, for
    both forms; compressed and uncompressed forms decode to the same points; GT through e(P_i, Q_i)."""
    import torch
    n = 1 << 14
    g1, g2 = eng.generators()
    P = torch.from_numpy(eng.g1_scalar_mul(g1, scalars("wP", n))).cuda()
    Q = torch.from_numpy(eng.g2_scalar_mul(g2, scalars("wQ", n))).cuda()
    P[5].zero_()
    Q[9].zero_()                                         # infinity rows
    for X, marshal, unmarshal, raw_w in ((P, eng.g1_marshal, eng.g1_unmarshal, 64), (Q, eng.g2_marshal, eng.g2_unmarshal, 128)):
        raw, comp = marshal(X), marshal(X, compressed=True)
        assert raw.shape == (n, raw_w) and comp.shape == (n, raw_w // 2)
        for enc in (raw, comp):
            back, ok = unmarshal(enc, elem_bytes=enc.shape[1])
            assert bool(ok.all()) and torch.equal(back, X)
        assert int((comp[:, 0] >> 6).min()) >= 1          # every compressed row carries a flag
    m = 2048
    gt = eng.pair_batch(P[:m].contiguous(), Q[:m].contiguous())
    back, ok = eng.gt_unmarshal(eng.gt_marshal(gt))
    assert bool(ok.all()) and torch.equal(back, gt)
    assert eng.gt_marshal(gt)[5].cpu().numpy().tobytes() == bytes(383) + b"\x01"      # e(inf, Q) = 1


# ---------------------------------------------------------------------------------------- hash to curve (§8 f-1)
def test_hash_to_curve_golden(eng):
    from gopairingbasedcryptography_amd import hash_to
    g = load_golden("hash_to_curve.json")
    dsts = {k: v.encode() for k, v in g["dsts"].items()}
    for key, fn in (("g1", hash_to.hash_to_g1), ("g2", hash_to.hash_to_g2)):
        for dk in sorted({c["dst"] for c in g[key]}):
            cs = [c for c in g[key] if c["dst"] == dk]
            out = fn([c["msg"].encode() for c in cs], dsts[dk])
            for i, c in enumerate(cs):
                assert out[i].tobytes().hex() == c["point"], (key, dk, c["msg"])
    rows = cat([o.fp_to_mont_bytes(int(c["u"][0])).hex() + o.fp_to_mont_bytes(int(c["u"][1])).hex() for c in g["g1_fields"]])
    out = eng.map_to_g1(rows)
    for i, c in enumerate(g["g1_fields"]):
        assert out[i].tobytes().hex() == c["point"], ("g1_fields", i)
    f2 = lambda v: o.f2_to_bytes((int(v[0]), int(v[1]))).hex()
    out = eng.map_to_g2(cat([f2(c["u"][0]) + f2(c["u"][1]) for c in g["g2_fields"]]))
    for i, c in enumerate(g["g2_fields"]):
        assert out[i].tobytes().hex() == c["point"], ("g2_fields", i)
    # the reference's four entry points
    assert hash_to.ToG1("user@example.com").tobytes().hex() == [c for c in g["g1"] if c["msg"] == "user@example.com" and c["dst"] == "string_g1"][0]["point"]
    assert hash_to.BytesToG1(b"abc").tobytes().hex() == [c for c in g["g1"] if c["msg"] == "abc" and c["dst"] == "bytes_g1"][0]["point"]
    assert hash_to.ToG2("abc").tobytes().hex() == [c for c in g["g2"] if c["msg"] == "abc" and c["dst"] == "string_g2"][0]["point"]


def test_hash_to_field_on_device(eng):
    """expand_message_xmd + reduction on the device (csrc/xmd29.hip.hpp) against the hashlib restatement that the RFC 9380 K.1
    vectors pin (tests/test_hash_to_curve.py): message lengths around every SHA-256 block and padding boundary, empty and long
    messages, DSTs of 0 / 1 / 28 / 255 bytes (256 is refused, as gnark does), both element counts; host and device buffers; and the whole
    hash-to-curve against host hashing + device map."""
    import torch
    from gopairingbasedcryptography_amd import hash_to
    rng = np.random.default_rng(2380)
    lens = [0, 1, 2, 3, 4, 5, 31, 32, 33, 50, 51, 52, 53, 54, 55, 56, 57, 63, 64, 65, 100, 114, 115, 116, 119, 120, 127, 128, 129, 255, 256, 1000, 4097]
    msgs = [rng.bytes(n) for n in lens] + [b"abc", b"", b"abcdef0123456789"]
    mont = lambda v: (v * (1 << 256) % hash_to.P_MOD).to_bytes(32, "little")
    for dst in (b"", b"d", hash_to.DST_STRING_G1, b"Q" * 255):
        for count in (2, 4):
            want = np.frombuffer(b"".join(mont(v) for m in msgs for v in hash_to.hash_to_field(m, dst, count)), dtype=np.uint8).reshape(len(msgs), count * 32)
            assert (eng.hash_to_field(msgs, dst, count) == want).all(), (len(dst), count)
        assert (eng.hash_to_g1(msgs, dst) == hash_to.hash_to_g1_via_host_fields(msgs, dst)).all()
    assert (eng.hash_to_g2(msgs, hash_to.DST_BYTES_G2) == hash_to.hash_to_g2_via_host_fields(msgs, hash_to.DST_BYTES_G2)).all()
    # device-resident messages and offsets; a table that points outside the buffer is clamped (no fault), not trusted
    data = torch.from_numpy(np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()).cuda()
    off = torch.tensor(np.concatenate([[0], np.cumsum([len(m) for m in msgs])]), dtype=torch.int64).cuda()
    want = eng.hash_to_field(msgs, hash_to.DST_BYTES_G1, 2)
    assert (eng.hash_to_field(data, hash_to.DST_BYTES_G1, 2, msg_off=off).cpu().numpy() == want).all()
    assert (eng.hash_to_g1(data, hash_to.DST_BYTES_G1, msg_off=off).cpu().numpy() == eng.hash_to_g1(msgs, hash_to.DST_BYTES_G1)).all()
    bad = off.clone()
    bad[-1] = 1 << 40
    got = eng.hash_to_field(data, hash_to.DST_BYTES_G1, 2, msg_off=bad).cpu().numpy()
    assert (got[:-1] == want[:-1]).all()                       # the last message was cut at the end of the buffer: same bytes here
    assert (got[-1] == want[-1]).all()
    with pytest.raises(ValueError):
        eng.hash_to_field(np.frombuffer(b"abc", dtype=np.uint8), b"d", 2, msg_off=np.array([0, 5], dtype=np.uint64))
    with pytest.raises(ValueError):
        eng.hash_to_field([b"abc"], b"d", 3)
    # an empty DST passed as NULL / 0 through the raw C ABI (what the Go shim does: unsafe.SliceData of an empty slice may be nil)
    import ctypes
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    data = np.frombuffer(b"abcdef", dtype=np.uint8).copy()
    offs = np.array([0, 3, 6], dtype=np.uint64)
    out = np.zeros((2, 64), dtype=np.uint8)
    _lib.check(lib.gpbc_hash_to_g1(data.ctypes.data_as(ctypes.c_void_p), offs.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(2), None, ctypes.c_size_t(0),
                                   out.ctypes.data_as(ctypes.c_void_p)))
    assert (out == eng.hash_to_g1([b"abc", b"def"], b"")).all()
    assert lib.gpbc_hash_to_g1(data.ctypes.data_as(ctypes.c_void_p), offs.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(2), None, ctypes.c_size_t(5),
                               out.ctypes.data_as(ctypes.c_void_p)) < 0          # NULL with a length is an error, not a crash
    for fn in (eng.hash_to_g1, eng.hash_to_g2, eng.hash_to_field):      # gnark's ExpandMsgXmd: "invalid domain size" above 255 bytes; the
        with pytest.raises(ValueError):                                 # Go shim answers the same (gpbcbn254.go), and so does this front end
            fn([b"abc"], b"R" * 256)
    assert eng.hash_to_g1([], b"d").shape == (0, 64)


def test_hash_to_curve_large_batch_properties(eng):
    """Size-independent properties at 2^13 messages: every point passes the curve / subgroup checks of the independent
    unmarshal kernels, the map is deterministic, and BLS sign / verify closes over hashed message points:
    e(pk, H(m)) == e(g1, [sk]H(m))  (signature/bls01_signature/bls_signature.go:58-89 with the real hash)."""
    from gopairingbasedcryptography_amd import hash_to
    n = 1 << 13
    msgs = [b"message %d" % i for i in range(n)]
    H1 = hash_to.hash_to_g1(msgs, hash_to.DST_BYTES_G1)
    H2 = hash_to.hash_to_g2(msgs, hash_to.DST_BYTES_G2)
    for pts, marshal, unmarshal in ((H1, eng.g1_marshal, eng.g1_unmarshal), (H2, eng.g2_marshal, eng.g2_unmarshal)):
        back, ok = unmarshal(marshal(pts))
        assert ok.all() and (back == pts).all()
        assert len({r.tobytes() for r in pts}) == n and pts.any(axis=1).all()        # distinct, none at infinity
    assert (hash_to.hash_to_g2(msgs[:64], hash_to.DST_BYTES_G2) == H2[:64]).all()
    # calls of up to 16 384 messages run one message per QUAD of lanes (the two maps side by side, G2's cofactor clearing three products
    # wide), larger ones one message per lane: the same messages through both, and a sample against the big-integer restatement
    big = msgs + [b"and %d more" % i for i in range(16385 - n)]
    L1, L2 = hash_to.hash_to_g1(big, hash_to.DST_BYTES_G1), hash_to.hash_to_g2(big, hash_to.DST_BYTES_G2)
    assert (L1[:n] == H1).all() and (L2[:n] == H2).all()
    for i in (0, 1, n - 1, 16384):
        assert L1[i].tobytes() == o.g1_to_bytes(o.hash_to_g1(big[i], hash_to.DST_BYTES_G1)) and L2[i].tobytes() == o.g2_to_bytes(o.hash_to_g2(big[i], hash_to.DST_BYTES_G2))
    m = 256
    g1, g2 = eng.generators()
    sk = scalars("bls-sk", m)
    pk = eng.g1_scalar_mul(g1, sk)
    sig = eng.g2_scalar_mul(H2[:m], sk)
    lhs = eng.pair_batch(pk, H2[:m])
    rhs = eng.pair_batch(np.tile(g1, m), sig)
    assert (lhs == rhs).all()
    neg_sig = sig.copy().reshape(m, 128)
    P = np.stack([pk.reshape(m, 64), np.tile(g1, (m, 1))], axis=1).reshape(-1)
    # PairingCheck([pk, g1], [H(m), -sigma]) per message; a wrong message must fail
    from gopairingbasedcryptography_amd.sharding import shard_range  # noqa: F401  (import check only)
    negY = eng.g2_scalar_mul(sig, [o.R - 1] * m)
    Qv = np.stack([H2[:m], negY.reshape(m, 128)], axis=1).reshape(-1)
    ok = eng.pairing_check_batch(P, Qv, np.arange(0, 2 * m + 1, 2))
    assert ok.all()
    Qbad = np.stack([np.roll(H2[:m], 1, axis=0), negY.reshape(m, 128)], axis=1).reshape(-1)
    assert not eng.pairing_check_batch(P, Qbad, np.arange(0, 2 * m + 1, 2)).any()


def test_tiny_and_empty_batches(eng, oracle):
    """n = 1 and n = 0 through the newer entry points (grids of one partially filled wave; empty inputs are no-ops)."""
    import torch
    g1, g2 = eng.generators()
    k = scalars("tiny", 2)
    P = eng.g1_scalar_mul(g1, k[:32])
    Q = eng.g2_scalar_mul(g2, k[32:])
    want = oracle.pair_batch(P, Q, threads=1)
    assert (eng.multi_pair_fixed_q(P, Q) == want).all()
    assert (eng.multi_pair(torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda(), np.array([0, 1], dtype=np.uint64)).cpu().numpy() == want).all()
    fb = eng.FixedBase(P)
    assert (fb.mul(k[32:]) == oracle.g1_scalar_mul(P, k[32:], threads=1)).all()
    back, ok = eng.g2_unmarshal(eng.g2_marshal(Q, compressed=True), elem_bytes=64)
    assert ok.tolist() == [1] and (back == Q).all()
    assert eng.map_to_g1(np.zeros(64, dtype=np.uint8)).shape == (1, 64)
    assert (eng.gt_exp(want, [5]) == oracle.gt_exp(want, np.frombuffer((5).to_bytes(32, "little"), dtype=np.uint8))).all()
    empty = np.zeros(0, dtype=np.uint8)
    assert eng.g1_marshal(empty).shape == (0, 64) and eng.g2_unmarshal(empty)[0].shape == (0, 128)
    assert eng.map_to_g2(empty).shape == (0, 128) and eng.gt_marshal(empty).shape == (0, 384)
    assert eng.g1_scalar_mul(empty, empty).shape[0] == 0


def test_bucket_msm_against_scalar_multiplications(eng, oracle):
    """gpbc_g1/g2_scalar_mul_sum from 16 384 terms on runs the bucket (Pippenger) method of csrc/gpbc_msm.hip: both window sizes
    (12-bit below 2^17 terms, 16-bit from there), full-width scalars (values >= r included), zero scalars, points at infinity
    and repeated bases, against the sum of the engine's independent scalar multiplications and, on the small case, the oracle."""
    import ctypes
    import torch
    from gopairingbasedcryptography_amd import _lib
    def paths():                     # (bucket runs, skew fallbacks) so far — which way the sums went
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _lib.check(_lib.load().gpbc_msm_stats(ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value
    g1, g2 = eng.generators()
    rng = np.random.default_rng(1234)
    # full-width scalars at both window sizes; 128-bit scalars (the rho of BLS aggregate verification) and scalars below r (what every
    # reference call site passes: their top window holds digits 0..3 only) in the 12-bit range
    for n, kind in ((20001, "full"), (140003, "full"), (20001, "128bit"), (20001, "below_r")):
        K = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        if kind == "128bit":
            K[:, 16:] = 0
        if kind == "below_r":
            K[:, 31] &= 0x1F                                          # < 2^253 < r
        K[0] = 0; K[1] = 255 if kind == "full" else K[1]; K[2, 1:] = 0; K[5, 16:] = 0
        kb = rng.integers(0, 256, size=(n, 32), dtype=np.uint8); kb[:, 31] &= 0x1F
        dK, dkb = torch.from_numpy(K).cuda(), torch.from_numpy(kb).cuda()
        for gen, mul, summ, msm, w in ((g1, eng.g1_scalar_mul, eng.g1_sum, eng.g1_scalar_mul_sum, 64), (g2, eng.g2_scalar_mul, eng.g2_sum, eng.g2_scalar_mul_sum, 128)):
            B = mul(torch.from_numpy(gen).cuda(), dkb)
            B[3] = 0                                                  # infinity
            B[7] = B[6]; dK[7] = dK[6]                               # same base and scalar twice
            want = summ(mul(B, dK)).cpu().numpy()
            before = paths()
            got = msm(B, dK).cpu().numpy()
            assert (got == want).all(), (n, kind, w)
            after = paths()
            assert after[0] == before[0] + 1 and after[1] == before[1], ("random scalars must take the bucket path, not the fallback", n, kind, w, before, after)
            assert (msm(B.cpu().numpy(), dK.cpu().numpy()) == want).all(), (n, kind, w, "host entry")
            if kind != "full":
                continue
            if n < 50000:
                o_want = np.asarray(oracle.g1_sum(oracle.g1_scalar_mul(B.cpu().numpy(), dK.cpu().numpy(), threads=16)) if w == 64 else
                                    oracle.g2_sum(oracle.g2_scalar_mul(B.cpu().numpy(), dK.cpu().numpy(), threads=16))).reshape(-1)
                assert (got == o_want).all(), (n, w, "oracle")
            # skewed scalars: every term of a window in ONE bucket (all scalars equal; small integers; a single repeated value).
            # The engine must notice from the histogram and take the per-term path instead of one lane adding n points in a row
            # (seconds of one-wave latency) — same bits, and it must come back in well under a second.
            import time
            for name, Ks in (("all equal", np.repeat(K[9:10], n, axis=0)), ("small integers", np.pad((np.arange(n) % 3 + 1).astype(np.uint8)[:, None], ((0, 0), (0, 31)))),
                             ("one", np.pad(np.ones((n, 1), np.uint8), ((0, 0), (0, 31))))):
                dKs = torch.from_numpy(np.ascontiguousarray(Ks)).cuda()
                want_s = summ(mul(B, dKs)).cpu().numpy()
                before = paths()
                torch.cuda.synchronize(); t0 = time.perf_counter()
                got_s = msm(B, dKs).cpu().numpy()
                dt = time.perf_counter() - t0
                assert paths() == (before[0], before[1] + 1), ("skewed scalars must take the per-term path", n, w, name)
                assert (got_s == want_s).all(), (n, w, name)
                assert dt < 1.0, (n, w, name, dt)
                assert (msm(B.cpu().numpy(), Ks) == want_s).all(), (n, w, name, "host entry")


def test_profile_labels_are_kernel_names(eng, synth):
    """Every launch marks its stream under the launched kernel's own name (GPBC_LAUNCH, csrc/gpbc_common.hpp), so the
    per-kernel timing of gpbc_profile_end bills each kernel to itself: a small and a large call of every host-entry family
    report only kernels defined in csrc/, and a one-point G2 scalar multiplication reports the octet kernel it runs."""
    import ctypes
    import glob
    import os
    import re
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    src = "".join(open(f).read() for f in glob.glob(os.path.join(os.path.dirname(_lib.__file__), "csrc", "*.hip*")))
    defined = set(re.findall(r"(?:__global__|GPBC_KERNEL\w*) [^;{#]*?\b(k_\w+)\(", src))

    def profiled(fn):
        _lib.check(lib.gpbc_profile_begin(None))
        fn()
        names, ms, cnt, nk = ctypes.create_string_buffer(32 * 64), (ctypes.c_double * 64)(), (ctypes.c_int * 64)(), ctypes.c_int(0)
        _lib.check(lib.gpbc_profile_end(names, ms, cnt, 64, ctypes.byref(nk)))
        return [names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode() for i in range(nk.value)]

    P, Q = synth
    g1, g2 = eng.generators()
    big = 3000                                                   # above every combined / latency limit, below the pipelined one
    Pb, Qb = np.tile(P, (100, 1))[:6 * big], np.tile(Q, (100, 1))[:6 * big]
    GT = np.tile(eng.pair_batch(P[:8], Q[:8]), (625, 1))
    K = np.random.default_rng(7).integers(0, 256, 32 * 6 * big, dtype=np.uint8)

    def every_family():
        for n in (1, big):
            seg = np.arange(0, 2 * n + 1, 2, dtype=np.uint64)
            eng.pair_batch(Pb[:n], Qb[:n])
            eng.final_exp(eng.miller_loop(Pb[:n], Qb[:n]))
            eng.multi_pair(Pb[:2 * n], Qb[:2 * n], seg), eng.pairing_check_batch(Pb[:2 * n], Qb[:2 * n], seg)
            eng.multi_pair_fixed_q(Pb[:4 * (n // 2 + 1)], Qb[:4])
            eng.g1_scalar_mul(Pb[:n], K[:32 * n]), eng.g2_scalar_mul(Qb[:n], K[:32 * n])
            eng.g1_scalar_mul(g1, K[:32 * 6 * n]), eng.g2_scalar_mul(g2, K[:32 * 6 * n])
            eng.g1_scalar_mul_base(K[:32 * n]), eng.g2_scalar_mul_base(K[:32 * n])
            eng.FixedBase(g1).mul(K[:32 * 6 * n])
            eng.g1_sum(Pb[:n]), eng.g2_sum(Qb[:n])
            eng.g1_scalar_mul_sum(Pb[:6 * n], K[:32 * 6 * n])
            m = 5000 if n > 1 else 1                             # (GT.Exp's lane-pair kernel starts above two rounds of the chip)
            eng.gt_exp(GT[:m], K[:32 * m])
            eng.gt_mul(GT[:n], GT[:n]), eng.gt_div(GT[:n], GT[:n]), eng.gt_inverse(GT[:n])
            for m in (n, 6 * n):
                eng.g1_unmarshal(eng.g1_marshal(Pb[:m], compressed=True), elem_bytes=32)
                eng.g2_unmarshal(eng.g2_marshal(Qb[:m], compressed=True), elem_bytes=64)
                eng.gt_unmarshal(eng.gt_marshal(np.tile(GT, (4, 1))[:m]))
                eng.map_to_g1(np.zeros((m, 64), dtype=np.uint8)), eng.map_to_g2(np.zeros((m, 128), dtype=np.uint8))
                msgs = [b"m%d" % i for i in range(m)]
                eng.hash_to_g1(msgs, b"DST"), eng.hash_to_g2(msgs, b"DST"), eng.hash_to_field(msgs, b"DST", 4)
            eng.fp_mul(np.zeros(32 * n, dtype=np.uint8), np.zeros(32 * n, dtype=np.uint8))

    names = profiled(every_family)
    assert "(begin)" not in names and len(names) >= 30, names
    assert not [nm for nm in names if nm.split("<")[0] not in defined], (names, sorted(defined))
    assert profiled(lambda: eng.g2_scalar_mul(g2, K[:32])) == ["k_g2_scalar_mul_oct"]


def test_multi_pair_with_every_segment_empty(eng):
    """A multi-pairing or PairingCheck over segments that hold no pair at all (k = 1 and k = 3, no points): every product is GT's
    one and every check true, through the Python wrappers and through the raw ABI with null point pointers.  (Such a call has no
    pairs for the combined latency route and must take the device-block route.)"""
    import ctypes
    from gopairingbasedcryptography_amd import _lib
    lib = _lib.load()
    g1, g2 = eng.generators()
    one = eng.pair_batch(np.zeros(64, dtype=np.uint8), g2)[0]
    none_p, none_q = np.zeros((0, 64), dtype=np.uint8), np.zeros((0, 128), dtype=np.uint8)
    for k in (1, 3):
        seg = np.zeros(k + 1, dtype=np.uint64)
        assert (eng.multi_pair(none_p, none_q, seg) == one).all(), k
        assert eng.pairing_check_batch(none_p, none_q, seg).all(), k
        out, ok = np.zeros((k, 384), dtype=np.uint8), np.zeros(k, dtype=np.uint8)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t(k)
        _lib.check(lib.gpbc_multi_pair(None, None, vp(seg.ctypes.data), sz, vp(out.ctypes.data)))
        _lib.check(lib.gpbc_pairing_check(None, None, vp(seg.ctypes.data), sz, vp(ok.ctypes.data)))
        assert (out == one).all() and ok.all(), k
