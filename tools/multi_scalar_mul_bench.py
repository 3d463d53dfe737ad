"""Segmented G1 / G2 multi-scalar multiplication (gpbc_g*_multi_scalar_mul_dev) on HBM-resident data against the route the engine had
before it to the same bytes — gpbc_g*_scalar_mul_batch_dev over all n terms, then log2(m) rounds of gpbc_g*_add_batch_dev on
re-sliced buffers.  One process, one device; every shape is warmed up first, then the two routes alternate repetition by repetition,
timed with HIP events on the current stream; min / median / max and all samples are kept.  A route is called faster only where its
slowest repetition beats the other route's fastest.

  * entry against the composed route: 2^16 segments x 16 terms and 2^12 x 64, both groups, one scalar per term and one shared list;
    the outputs are compared for equality;
  * GMSM_GROUP 4 (the in-tree library) against a variant library built with another group size, G1, same buffers:
        bash tools/build_variant.sh gmsm8 -DGMSM_GROUP=8        then        --variant variants/libgpbc_gmsm8.so
  * k_g1_multi_scalar_mul at two waves per SIMD (in-tree) against a copy of csrc/ with that kernel declared GPBC_KERNEL_G1 (three
    waves, 168 VGPRs), built with GPBC_SRC=... tools/build_variant.sh: --waves3 variants/libgpbc_gmsmw3.so
  * waters11.decrypt_batch with msm False / True at 2^14 ciphertexts x 16 rows;
  * lw11.decrypt_batch against lw11.decrypt_batch_msm at 2^14 ciphertexts under one 16-row policy.
Writes one JSON document (profiles/multi_scalar_mul.json records a run).

    python tools/multi_scalar_mul_bench.py [--reps 5] [--variant LIB] [--out FILE] [--skip-planners]"""
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

from gopairingbasedcryptography_amd import _lib, bn254, lw11, waters11  # noqa: E402

P, SZ = ctypes.c_void_p, ctypes.c_size_t
# Fp-product equivalents per term (a Jacobian doubling ~ 7, a mixed addition ~ 11): doublings, additions, table
PAPER = {"g1": {"doublings": 910, "additions": 715, "table": 200}, "g2": {"doublings": 460, "additions": 730, "table": 300}}


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stats(ts):
    return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts), "all_ms": ts}


def verdict(new, old):
    """'new' / 'old' where that route's slowest repetition beats the other's fastest, else 'neither'"""
    return "new" if max(new) < min(old) else "old" if max(old) < min(new) else "neither"


def alternate(old, new, reps):
    t_old, t_new = [], []
    for _ in range(reps):
        t_old.append(timed(old))
        t_new.append(timed(new))
    return t_old, t_new


def points(g2, n, seed):
    """n points [a_i] G made by the engine's scalar multiplication of the generator, and n random 256-bit scalars"""
    rng = np.random.default_rng(seed)
    a = dev(rng.integers(0, 256, size=(n, 32), dtype=np.uint8))
    gen = dev(bn254.generators()[1 if g2 else 0])
    x = (bn254.g2_scalar_mul if g2 else bn254.g1_scalar_mul)(gen, a.reshape(-1))
    return x, dev(rng.integers(0, 256, size=(n, 32), dtype=np.uint8))


def composed(g2, x, k, n_seg, m, tmp):
    w = 128 if g2 else 64
    mul, add = (bn254.g2_scalar_mul, bn254.g2_add) if g2 else (bn254.g1_scalar_mul, bn254.g1_add)
    cur = mul(x.reshape(-1), k.reshape(-1), out=tmp).reshape(n_seg, m, w)
    while m > 1:
        cur = add(cur[:, 0::2].contiguous().reshape(-1), cur[:, 1::2].contiguous().reshape(-1)).reshape(n_seg, m // 2, w)
        m //= 2
    return cur.reshape(n_seg, w)


def entry(lib, g2, x, k, nk, table, n, n_seg, out, ws):
    fn = lib.gpbc_g2_multi_scalar_mul_dev if g2 else lib.gpbc_g1_multi_scalar_mul_dev
    rc = fn(P(x.data_ptr()), P(k.data_ptr()), SZ(nk), P(table.data_ptr()), SZ(n), SZ(n_seg), P(out.data_ptr()), P(ws.data_ptr()), SZ(ws.numel()),
            P(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise RuntimeError("gpbc_g%d_multi_scalar_mul_dev: %d" % (2 if g2 else 1, rc))
    return out


def load_variant(path):
    """another build of the library in the same process (its own handle, initialised on the same device): only the entries used here"""
    v = ctypes.CDLL(os.path.abspath(path))
    v.gpbc_init.restype, v.gpbc_init.argtypes = ctypes.c_int, [ctypes.c_int]
    v.gpbc_multi_scalar_mul_workspace_bytes.restype, v.gpbc_multi_scalar_mul_workspace_bytes.argtypes = SZ, [SZ, SZ, ctypes.c_int]
    for name in ("gpbc_g1_multi_scalar_mul_dev", "gpbc_g2_multi_scalar_mul_dev"):
        getattr(v, name).restype, getattr(v, name).argtypes = ctypes.c_int, [P, P, SZ, P, SZ, SZ, P, P, SZ, P]
    if v.gpbc_init(0) != 0:
        raise RuntimeError("gpbc_init of %s failed" % path)
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--variant", default=None, help="a library built with another GMSM_GROUP (tools/build_variant.sh)")
    ap.add_argument("--variant-group", type=int, default=8)
    ap.add_argument("--waves3", default=None, help="a library whose k_g1_multi_scalar_mul is built for three waves per SIMD (GPBC_KERNEL_G1)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-planners", action="store_true")
    args = ap.parse_args()
    bn254.init(0)
    lib = _lib.load()
    variant = load_variant(args.variant) if args.variant else None
    waves3 = load_variant(args.waves3) if args.waves3 else None
    doc = {"reps": args.reps, "device": torch.cuda.get_device_name(0), "paper_fp_products_per_term": PAPER, "entry_vs_composed": {}, "group_size_g1": {}, "occupancy_g1": {}}
    for g, c in PAPER.items():
        c["expected_ratio_from_shared_doublings"] = sum(c[k] for k in ("doublings", "additions", "table")) / (c["doublings"] / 4 + c["additions"] + c["table"])
    for g2 in (False, True):
        w, name = (128, "g2") if g2 else (64, "g1")
        for n_seg, m in ((1 << 16, 16), (1 << 12, 64)):
            n = n_seg * m
            x, k = points(g2, n, 100 + m + int(g2))
            table = dev(np.arange(0, n + 1, m, dtype=np.int64))
            out = torch.empty((n_seg, w), dtype=torch.uint8, device="cuda")
            tmp = torch.empty((n, w), dtype=torch.uint8, device="cuda")
            ws = torch.empty(max(lib.gpbc_multi_scalar_mul_workspace_bytes(n, n_seg, int(g2)), 1), dtype=torch.uint8, device="cuda")
            k_list = k[:m].contiguous()
            k_tiled = k_list.repeat(n_seg, 1).contiguous()
            for form, nk, kk, kc in (("one scalar per term", n, k, k), ("shared list", m, k_list, k_tiled)):
                new = lambda: entry(lib, g2, x, kk, nk, table, n, n_seg, out, ws)
                old = lambda: composed(g2, x, kc, n_seg, m, tmp)
                same = bool((new() == old()).all())                              # warm-up, and the bytes agree
                torch.cuda.synchronize()
                t_old, t_new = alternate(old, new, args.reps)
                rec = {"group": name, "n_seg": n_seg, "terms_per_segment": m, "scalars": form, "same_bytes": same, "entry": stats(t_new), "composed": stats(t_old),
                       "speedup_of_medians": statistics.median(t_old) / statistics.median(t_new), "faster": verdict(t_new, t_old),
                       "M_terms_per_s": n / statistics.median(t_new) / 1e3}
                doc["entry_vs_composed"]["%s %dx%d %s" % (name, n_seg, m, form)] = rec
                print("%s %d x %d, %s: entry %.2f ms, composed %.2f ms: %.2fx, faster: %s, same bytes %s" % (
                    name, n_seg, m, form, rec["entry"]["median_ms"], rec["composed"]["median_ms"], rec["speedup_of_medians"], rec["faster"], same), flush=True)
            if variant is not None and not g2:
                vws = torch.empty(max(variant.gpbc_multi_scalar_mul_workspace_bytes(n, n_seg, 0), 1), dtype=torch.uint8, device="cuda")
                vout = torch.empty_like(out)
                a = lambda: entry(lib, False, x, k, n, table, n, n_seg, out, ws)
                b = lambda: entry(variant, False, x, k, n, table, n, n_seg, vout, vws)
                same = bool((a() == b()).all())
                torch.cuda.synchronize()
                t_a, t_b = alternate(a, b, args.reps)
                v = verdict(t_b, t_a)
                doc["group_size_g1"]["%dx%d" % (n_seg, m)] = {"same_bytes": same, "group_4": stats(t_a), "group_%d" % args.variant_group: stats(t_b),
                                                             "faster": {"new": "group_%d" % args.variant_group, "old": "group_4", "neither": "neither"}[v]}
                print("g1 %d x %d: group 4 %.2f ms, group %d %.2f ms, same bytes %s" % (n_seg, m, statistics.median(t_a), args.variant_group, statistics.median(t_b), same), flush=True)
                del vws, vout
            if waves3 is not None and not g2:
                vws = torch.empty(max(waves3.gpbc_multi_scalar_mul_workspace_bytes(n, n_seg, 0), 1), dtype=torch.uint8, device="cuda")
                vout = torch.empty_like(out)
                a = lambda: entry(lib, False, x, k, n, table, n, n_seg, out, ws)
                b = lambda: entry(waves3, False, x, k, n, table, n, n_seg, vout, vws)
                same = bool((a() == b()).all())
                torch.cuda.synchronize()
                t_a, t_b = alternate(a, b, args.reps)
                doc["occupancy_g1"]["%dx%d" % (n_seg, m)] = {"same_bytes": same, "waves_2": stats(t_a), "waves_3": stats(t_b),
                                                            "faster": {"new": "waves_3", "old": "waves_2", "neither": "neither"}[verdict(t_b, t_a)]}
                print("g1 %d x %d: 2 waves per SIMD %.2f ms, 3 waves %.2f ms, same bytes %s" % (n_seg, m, statistics.median(t_a), statistics.median(t_b), same), flush=True)
                del vws, vout
            del x, k, out, tmp, ws, k_tiled
            lib.gpbc_release_workspaces()
    if not args.skip_planners:
        n, R = 1 << 14, 16
        d = torch.device("cuda", 0)
        from waters11_fixture import Instance as W11, at_size_policies
        pols, key = at_size_policies(n)
        inst = W11(bn254, key, pols, rows=R, dev=d, tag="bench")
        pad = waters11.pad_policies(pols, rows=R)
        old = lambda: waters11.decrypt_batch(bn254, inst.key, pad, inst.c, inst.c_prime, inst.cx, inst.dx)
        new = lambda: waters11.decrypt_batch(bn254, inst.key, pad, inst.c, inst.c_prime, inst.cx, inst.dx, msm=True)
        (o0, k0), (o1, k1) = old(), new()
        same = bool((o0 == o1).all()) and bool((k0 == k1).all())
        torch.cuda.synchronize()
        t_old, t_new = alternate(old, new, args.reps)
        doc["waters11_2_14_x_16"] = {"ciphertexts": n, "rows": R, "same_bytes": same, "msm_false": stats(t_old), "msm_true": stats(t_new),
                                     "faster": {"new": "msm_true", "old": "msm_false", "neither": "neither"}[verdict(t_new, t_old)]}
        print("waters11 2^14 x 16: msm False %.2f ms, True %.2f ms, same bytes %s" % (statistics.median(t_old), statistics.median(t_new), same), flush=True)
        del inst, o0, o1
        lib.gpbc_release_workspaces()
        from lw11_fixture import Instance as L11, threshold_policy
        m, rho = threshold_policy(R, R)
        inst = L11(bn254, m, rho, rho, n_ct=n, dev=d, tag="bench")
        rows, wts = lw11.reconstruction_weights(m, rho, inst.user_attrs)
        folded = lw11.fold_key(bn254, rows, wts, inst.h_gid, inst.k_by_row)
        old = lambda: lw11.decrypt_batch(bn254, folded, inst.c0, inst.c1, inst.c2, inst.c3)
        new = lambda: lw11.decrypt_batch_msm(bn254, folded, inst.h_gid, inst.c0, inst.c1, inst.c2, inst.c3)
        o0, o1 = old(), new()
        same = bool((o0 == o1).all()) and bool((o1 == inst.msgs).all())
        torch.cuda.synchronize()
        t_old, t_new = alternate(old, new, args.reps)
        doc["lw11_2_14_x_16"] = {"ciphertexts": n, "rows": R, "same_bytes_and_messages": same, "decrypt_batch": stats(t_old), "decrypt_batch_msm": stats(t_new),
                                 "faster": {"new": "decrypt_batch_msm", "old": "decrypt_batch", "neither": "neither"}[verdict(t_new, t_old)]}
        print("lw11 2^14 x 16: decrypt_batch %.2f ms, decrypt_batch_msm %.2f ms, same bytes %s" % (statistics.median(t_old), statistics.median(t_new), same), flush=True)
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
