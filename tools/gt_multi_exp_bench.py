"""Segmented GT multi-exponentiation (gpbc_gt_multi_exp_dev) on HBM-resident data against the route the engine had before it to
the same bytes — gpbc_gt_exp_batch_dev over all n elements, then log2(m) rounds of gpbc_gt_mul_batch_dev on re-sliced buffers —
alternated repetition by repetition after a warm-up, timed with HIP events on the current stream; medians, samples kept.
Shapes: 2^16 segments x 16 factors, 2^12 x 64, both with one exponent per element.  Also gt_prod of 2^20 elements in one segment
beside gt_mul of 2^20, and lw11.decrypt_batch at 2^14 ciphertexts x 16 rows with its per-kernel split (gpbc_profile_begin / _end).
Writes one JSON document (profiles/gt_multi_exp.json records a run).

    python tools/gt_multi_exp_bench.py [--reps 5] [--out FILE] [--skip-lw11]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopairingbasedcryptography_amd import _lib, bn254, lw11  # noqa: E402

GT = 384
PAPER = {"parent_sq_equiv_per_factor": 252 + 77 * 2.34, "straus4_sq_equiv_per_factor": 63 + 77.25 * 2.34}


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def inputs(n, seed):
    """n pairing values e(g1, g2)^a_i and n random 256-bit exponents"""
    g1, g2 = bn254.generators()
    e = bn254.pair_batch(g1, g2)
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 31] &= 0x1F
    x = bn254.gt_exp(dev(np.tile(e.reshape(1, GT), (n, 1))).reshape(-1), dev(a).reshape(-1))
    return x, dev(rng.integers(0, 256, size=(n, 32), dtype=np.uint8))


def parent_route(x, k, n_seg, m, tmp):
    cur = bn254.gt_exp(x.reshape(-1), k.reshape(-1), out=tmp).reshape(n_seg, m, GT)
    while m > 1:
        cur = bn254.gt_mul(cur[:, 0::2].contiguous().reshape(-1), cur[:, 1::2].contiguous().reshape(-1)).reshape(n_seg, m // 2, GT)
        m //= 2
    return cur.reshape(n_seg, GT)


def profile(fn):
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.gpbc_profile_begin(stream))
    fn()
    names = ctypes.create_string_buffer(64 * 32)
    ms, cnt, nk = (ctypes.c_double * 64)(), (ctypes.c_int * 64)(), ctypes.c_int(0)
    _lib.check(lib.gpbc_profile_end(names, ms, cnt, 64, ctypes.byref(nk)))
    return {names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode(): {"ms": ms[i], "launches": cnt[i]} for i in range(nk.value)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-lw11", action="store_true")
    args = ap.parse_args()
    bn254.init(0)
    lib = _lib.load()
    doc = {"reps": args.reps, "device": torch.cuda.get_device_name(0), "paper": PAPER, "shapes": {}}
    doc["paper"]["ratio"] = PAPER["parent_sq_equiv_per_factor"] / PAPER["straus4_sq_equiv_per_factor"]
    for n_seg, m in ((1 << 16, 16), (1 << 12, 64)):
        n = n_seg * m
        x, k = inputs(n, 100 + m)
        table = dev(np.arange(0, n + 1, m, dtype=np.int64))
        out = torch.empty((n_seg, GT), dtype=torch.uint8, device="cuda")
        tmp = torch.empty((n, GT), dtype=torch.uint8, device="cuda")
        ws = torch.empty(max(lib.gpbc_gt_multi_exp_workspace_bytes(n, n_seg), 1), dtype=torch.uint8, device="cuda")
        P, SZ = ctypes.c_void_p, ctypes.c_size_t

        def new():                                                           # the C entry itself: the table is already on the device
            _lib.check(lib.gpbc_gt_multi_exp_dev(P(x.data_ptr()), P(k.data_ptr()), SZ(n), P(table.data_ptr()), SZ(n), SZ(n_seg), P(out.data_ptr()),
                                                 P(ws.data_ptr()), SZ(ws.numel()), P(torch.cuda.current_stream().cuda_stream)))
            return out
        old = lambda: parent_route(x, k, n_seg, m, tmp)
        same = bool((new() == old()).all())                                  # warm-up, and the bytes agree
        torch.cuda.synchronize()
        t_new, t_old = [], []
        for _ in range(args.reps):
            t_old.append(timed(old))
            t_new.append(timed(new))
        mn, mo = statistics.median(t_new), statistics.median(t_old)
        spread = max(t_old) - min(t_old)
        doc["shapes"]["%dx%d" % (n_seg, m)] = {
            "n_seg": n_seg, "factors_per_segment": m, "same_bytes": same, "gt_multi_exp_ms": mn, "gt_multi_exp_ms_all": t_new,
            "parent_route_ms": mo, "parent_route_ms_all": t_old, "parent_spread_ms": spread, "speedup": mo / mn,
            "not_slower_within_parent_spread": mn <= mo + spread, "M_factors_per_s": n / mn / 1e3,
            "kernels": profile(new), "parent_kernels": profile(old)}
        print("%d x %d: gt_multi_exp %.2f ms, parent route %.2f ms (spread %.2f): %.2fx, same bytes %s" % (n_seg, m, mn, mo, spread, mo / mn, same), flush=True)
        del x, k, out, tmp, ws
        lib.gpbc_release_workspaces()
    # plain product of 2^20 elements in one segment beside the elementwise product of 2^20
    n = 1 << 20
    x, _ = inputs(n, 7)
    y = x.flip(0).contiguous()
    prod = lambda: bn254.gt_prod(x.reshape(-1))
    mul = lambda: bn254.gt_mul(x.reshape(-1), y.reshape(-1))
    prod(), mul()
    torch.cuda.synchronize()
    t_prod, t_mul = [], []
    for _ in range(args.reps):
        t_mul.append(timed(mul))
        t_prod.append(timed(prod))
    mp, mm = statistics.median(t_prod), statistics.median(t_mul)
    doc["gt_prod_2_20"] = {"n": n, "gt_prod_ms": mp, "gt_prod_ms_all": t_prod, "gt_prod_GBs_read": n * GT / mp / 1e6, "gt_mul_ms": mm, "gt_mul_ms_all": t_mul,
                           "gt_mul_GBs_read": 2 * n * GT / mm / 1e6, "kernels": profile(prod)}
    print("gt_prod 2^20 in one segment: %.3f ms = %.0f GB/s read; gt_mul 2^20: %.3f ms = %.0f GB/s read" % (mp, n * GT / mp / 1e6, mm, 2 * n * GT / mm / 1e6), flush=True)
    del x, y
    lib.gpbc_release_workspaces()
    if not args.skip_lw11:
        from lw11_fixture import Instance, threshold_policy
        n, R = 1 << 14, 16
        m, rho = threshold_policy(R, R)
        inst = Instance(bn254, m, rho, rho, n_ct=n, dev=torch.device("cuda", 0), tag="bench")
        rows, w = lw11.reconstruction_weights(m, rho, inst.user_attrs)
        folded = lw11.fold_key(bn254, rows, w, inst.h_gid, inst.k_by_row)
        run = lambda: lw11.decrypt_batch(bn254, folded, inst.c0, inst.c1, inst.c2, inst.c3)
        ok = bool((run() == inst.msgs).all())
        torch.cuda.synchronize()
        ts = [timed(run) for _ in range(args.reps)]
        med = statistics.median(ts)
        kern = profile(run)
        group = lambda name: "multi_exp" if name.startswith(("k_gt_multi_exp", "k_gt_prod")) else "divisions" if name.startswith("k_gt_binary") else "pairings"
        split = {}
        for name, v in kern.items():
            split[group(name)] = split.get(group(name), 0.0) + v["ms"]
        doc["lw11_2_14_x_16"] = {"ciphertexts": n, "rows": R, "messages_recovered": ok, "ms": med, "ms_all": ts, "ciphertexts_per_s": n / med * 1e3,
                                 "split_ms": split, "kernels": kern}
        print("lw11.decrypt_batch 2^14 x 16 rows: %.2f ms = %.0f ciphertexts/s, split %s, messages %s" % (med, n / med * 1e3, split, ok), flush=True)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
