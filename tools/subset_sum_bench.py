"""Bit-selected sums over a fixed set (gpbc_subset_sum_dev, include/gpbc_bn254_subset.h) on HBM-resident data against the routes the
engine had before it to the same bytes, 256-bit masks (SHA-256 digests' shape) over one table of 256 points and an offset:

  * the table route: gpbc_subset_sum_dev, n = 2^16 and 2^20, G1 and G2 — kernel time between device events and items/s;
  * the gather route: the selected points of every item (and the offset) gathered on the device by index_select, then
    gpbc_g*_multi_scalar_mul_dev without scalars (g*_sum_segments) over the gathered points.  Timed: the gather and the sums; the
    index list (which bits are set) is made before the clock starts, in the route's favour.  n = 2^16, and 2^20 unless the gathered
    points do not fit (then said so, with the largest power of two that does);
  * FixedBase.msm with 0 / 1 scalars over the same 257 points (gpbc_fixed_base_msm_dev), n = 2^16 and the largest n <= 2^20 whose
    8 KiB of scalars per item fit;
  * the table build (gpbc_subset_table_create_dev: device events around the kernel, and the whole call with its hipMalloc);
  * waters05.keygen_batch / encrypt_batch / decrypt_batch at 2^16 identities, device resident.
The output bytes of the routes are compared before any time is reported; every shape is warmed up first, then timed `--reps` times
(min / median / max and all samples kept).  One process, one device.  Writes one JSON document (profiles/subset_sum.json records a run).

    python tools/subset_sum_bench.py [--reps 5] [--max-log-n 20] [--out FILE] [--skip-planner]"""
import argparse
import ctypes
import datetime
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopairingbasedcryptography_amd import _lib, bn254, waters05  # noqa: E402

P, SZ = ctypes.c_void_p, ctypes.c_size_t
NBITS, W = 256, 32


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def stats(ts):
    return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts), "all_ms": ts}


def measure(fn, reps):
    fn()
    torch.cuda.synchronize()
    return stats([timed(fn) for _ in range(reps)])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return P(torch.cuda.current_stream().cuda_stream)


def rand_rows(rng, n, width):
    return dev(rng.integers(0, 256, size=(n, width), dtype=np.uint8))


def points(g2, n, rng):
    gen = dev(bn254.generators()[1 if g2 else 0])
    return (bn254.g2_scalar_mul if g2 else bn254.g1_scalar_mul)(gen, rand_rows(rng, n, 32).reshape(-1)).reshape(n, -1)


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s: %d %s" % (what, rc, _lib.load().gpbc_last_error()))


def mask_bits(masks):
    """[n, 256] 0 / 1 (uint8) of [n, 32] mask bytes, most significant bit of every byte first"""
    shifts = torch.arange(7, -1, -1, device="cuda", dtype=torch.int32)
    return ((masks[:, :, None].to(torch.int32) >> shifts) & 1).reshape(masks.shape[0], NBITS).to(torch.uint8)


def selection(masks):
    """(index of every selected point in [O, B_0 .. B_255], item by item; segment table): the offset is point 0 of every item"""
    n = masks.shape[0]
    bits = mask_bits(masks).bool()
    bits = torch.cat([torch.ones((n, 1), dtype=torch.bool, device="cuda"), bits], 1)
    idx = bits.nonzero()[:, 1].contiguous()
    seg = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), bits.sum(1).cumsum(0)]).contiguous()
    return idx, seg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-log-n", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-planner", action="store_true")
    args = ap.parse_args()
    bn254.init(0)
    lib = _lib.load()
    free, total = torch.cuda.mem_get_info()
    doc = {"reps": args.reps, "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "hbm_bytes": total, "nbits": NBITS,
           "paper_mixed_additions_per_item": {"table": 32, "gather": 128, "fixed_base_0_1": 128}, "routes": {}, "table_build": {}}
    rng = np.random.default_rng(2005)
    sizes = sorted({min(16, args.max_log_n), args.max_log_n})
    for g2 in (False, True):
        w, name = (128, "g2") if g2 else (64, "g1")
        bases, offset = points(g2, NBITS, rng), points(g2, 1, rng)
        # ---- the table and its build
        h = ctypes.c_void_p()

        def build():
            check(lib.gpbc_subset_table_create_dev(int(g2), P(bases.data_ptr()), NBITS, P(offset.data_ptr()), stream(), ctypes.byref(h)), "create_dev")
        kernel_ms, wall_ms = [], []
        for _ in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kernel_ms.append(timed(build))
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            lib.gpbc_subset_table_destroy(h)
        doc["table_build"][name] = {"table_bytes": lib.gpbc_subset_table_bytes(NBITS, int(g2)), "kernel": stats(kernel_ms[1:]), "whole_call_with_hipMalloc": stats(wall_ms[1:])}
        table = bn254.SubsetTable(bases, offset=offset, g2=g2)
        torch.cuda.synchronize()
        all_pts = torch.cat([offset, bases]).contiguous()                        # [257, w]: the offset is point 0
        fb = bn254.FixedBase(all_pts, g2=g2)
        for log_n in sizes:
            n = 1 << log_n
            rec = {"n": n}
            masks = rand_rows(rng, n, W)
            out = torch.empty((n, w), dtype=torch.uint8, device="cuda")
            assert lib.gpbc_subset_sum_workspace_bytes(table._h, n) == 0

            def new():
                check(lib.gpbc_subset_sum_dev(table._h, P(masks.data_ptr()), n, P(out.data_ptr()), None, 0, stream()), "subset_sum_dev")
            new()
            # ---- the gather route, on the largest power of two <= n that fits
            m = n
            got = None
            while m >= 1024:
                try:
                    idx, seg = selection(masks[:m])
                    total_pts = int(seg[-1])
                    gathered = torch.empty((total_pts, w), dtype=torch.uint8, device="cuda")
                    wsb = lib.gpbc_multi_scalar_mul_workspace_bytes(total_pts, m, int(g2))
                    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
                    got = torch.empty((m, w), dtype=torch.uint8, device="cuda")
                    break
                except torch.cuda.OutOfMemoryError:
                    idx = seg = gathered = ws = got = None
                    torch.cuda.empty_cache()
                    m //= 2
            sums = lib.gpbc_g2_multi_scalar_mul_dev if g2 else lib.gpbc_g1_multi_scalar_mul_dev

            def gather():
                torch.index_select(all_pts.view(torch.int64), 0, idx, out=gathered.view(torch.int64))      # rows as 8 / 16 words of 64 bits

            def sum_segments():
                check(sums(P(gathered.data_ptr()), None, 0, P(seg.data_ptr()), total_pts, m, P(got.data_ptr()), P(ws.data_ptr()), ws.numel(), stream()), "sum_segments")

            def old():
                gather()
                sum_segments()
            old()
            torch.cuda.synchronize()
            rec["gather_route_same_bytes"] = bool((got == out[:m]).all())
            rec["table"] = measure(new, args.reps)
            rec["table"]["M_items_per_s"] = n / rec["table"]["median_ms"] / 1e3
            g = {"n": m, "fits_at_n": m == n, "gathered_points": total_pts, "gathered_bytes": total_pts * w, "gather": measure(gather, args.reps),
                 "sum_segments": measure(sum_segments, args.reps), "gather_and_sum": measure(old, args.reps)}
            g["M_items_per_s"] = m / g["gather_and_sum"]["median_ms"] / 1e3
            rec["gather_route"] = g
            if m != n:                                                           # the table route at the common n
                small = measure(lambda: check(lib.gpbc_subset_sum_dev(table._h, P(masks.data_ptr()), m, P(out.data_ptr()), None, 0, stream()), "subset_sum_dev"), args.reps)
                rec["table_at_gather_n"] = small
                rec["ratio_table_over_gather_items_per_s"] = g["gather_and_sum"]["median_ms"] / small["median_ms"]
            else:
                rec["ratio_table_over_gather_items_per_s"] = g["gather_and_sum"]["median_ms"] / rec["table"]["median_ms"]
            del idx, seg, gathered, ws, got
            torch.cuda.empty_cache()
            # ---- FixedBase.msm with 0 / 1 scalars over [O, B_0 .. B_255]
            mf = n
            k = None
            while mf >= 1024:
                try:
                    k = torch.zeros((mf, NBITS + 1, 32), dtype=torch.uint8, device="cuda")
                    k[:, 0, 0] = 1
                    k[:, 1:, 0] = mask_bits(masks[:mf])
                    fwsb = lib.gpbc_fixed_base_msm_workspace_bytes(fb._h, mf)
                    fws = torch.empty(max(fwsb, 16), dtype=torch.uint8, device="cuda")
                    fout = torch.empty((mf, w), dtype=torch.uint8, device="cuda")
                    break
                except torch.cuda.OutOfMemoryError:
                    k = fws = fout = None
                    torch.cuda.empty_cache()
                    mf //= 2

            def fixed():
                check(lib.gpbc_fixed_base_msm_dev(fb._h, P(k.data_ptr()), mf, P(fout.data_ptr()), P(fws.data_ptr()), fws.numel(), stream()), "fixed_base_msm_dev")
            fixed()
            torch.cuda.synchronize()
            f = {"n": mf, "fits_at_n": mf == n, "scalar_bytes": k.numel(), "table_bytes": lib.gpbc_fixed_base_table_bytes(NBITS + 1, int(g2)),
                 "same_bytes": bool((fout == out[:mf]).all()), "msm": measure(fixed, args.reps)}
            f["M_items_per_s"] = mf / f["msm"]["median_ms"] / 1e3
            rec["fixed_base_0_1"] = f
            del k, fws, fout
            torch.cuda.empty_cache()
            doc["routes"]["%s 2^%d" % (name, log_n)] = rec
            print("%s n = 2^%d: table %.3f ms (%.1f M items/s); gather + sum at n = %d: %.3f ms, same bytes %s, ratio %.2fx; fixed base 0/1 at n = %d: %.3f ms, same bytes %s" % (
                name, log_n, rec["table"]["median_ms"], rec["table"]["M_items_per_s"], m, g["gather_and_sum"]["median_ms"], rec["gather_route_same_bytes"],
                rec["ratio_table_over_gather_items_per_s"], mf, f["msm"]["median_ms"], f["same_bytes"]), flush=True)
            del masks, out
        table.close()
        fb.close()
        lib.gpbc_release_workspaces()
    if not args.skip_planner:
        n = 1 << min(16, args.max_log_n)
        g1, g2gen = (dev(x) for x in bn254.generators())
        ui, u_prime = points(True, NBITS, rng), points(True, 1, rng)
        alpha = rand_rows(rng, 1, 32)
        g2_alpha, g1_alpha = bn254.g2_scalar_mul(g2gen, alpha.reshape(-1)), bn254.g1_scalar_mul(g1, alpha.reshape(-1))
        e_alpha = bn254.pair_batch(g1_alpha.reshape(-1), g2gen)
        masks, r, t = rand_rows(rng, n, W), rand_rows(rng, n, 32), rand_rows(rng, n, 32)
        e = bn254.pair_batch(g1, g2gen)
        messages = bn254.gt_exp(e.expand(n, 384).contiguous().reshape(-1), rand_rows(rng, n, 32).reshape(-1)).reshape(n, 384)
        table = waters05.hash_table(bn254, u_prime, ui)
        keys, cts = [None], [None]

        def keygen():
            keys[0] = waters05.keygen_batch(bn254, table, g2_alpha, masks, r)

        def encrypt():
            cts[0] = waters05.encrypt_batch(bn254, table, e_alpha, messages, masks, t)
        back = [None]

        def decrypt():
            back[0] = waters05.decrypt_batch(bn254, keys[0], *cts[0])
        rec = {"identities": n, "keygen_batch": measure(keygen, args.reps), "encrypt_batch": measure(encrypt, args.reps), "decrypt_batch": measure(decrypt, args.reps)}
        rec["hash_alone"] = measure(lambda: table.sum(masks), args.reps)
        rec["g2_scalar_mul_alone"] = measure(lambda: bn254.g2_scalar_mul(ui[:1].expand(n, 128).contiguous().reshape(-1), r.reshape(-1)), args.reps)
        rec["messages_returned"] = bool((back[0] == messages).all())
        doc["waters05_2_%d" % min(16, args.max_log_n)] = rec
        print("waters05 at %d identities: keygen %.2f ms, encrypt %.2f ms, decrypt %.2f ms; the hash alone %.3f ms, a G2 scalar multiplication of as many %.2f ms; messages returned %s" % (
            n, rec["keygen_batch"]["median_ms"], rec["encrypt_batch"]["median_ms"], rec["decrypt_batch"]["median_ms"], rec["hash_alone"]["median_ms"],
            rec["g2_scalar_mul_alone"]["median_ms"], rec["messages_returned"]), flush=True)
        table.close()
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text if not args.out else "written to " + args.out)


if __name__ == "__main__":
    main()
