#!/usr/bin/env python3
"""The device selection of common attributes and SW05 decryption from attribute rows measured on one MI355X: writes profiles/sw05_select.json.

  (a) fr_find_common alone on HBM-resident inputs at 2^16 items x (a = 24, m = 32, d = 16) — a shared set and a set per item — and at
      2^12 x (256, 256, 128): median of RUNS between device events;
  (b) sw05.decrypt_batch and sw05.decrypt_batch_large on 2^16 ciphertexts x 24 attributes against a key of 32, d = 16, in both input
      forms in one process — nested Python integers (host select_common: the code path as it was before the rows form) and attribute
      rows in HBM (fr_find_common) — whole calls by the wall clock, synchronised, median of RUNS; the messages of both are compared;
  (c) the device stages of the rows form on the planner's own intermediates (selection, Lagrange, scalar multiplications, multi-pairing,
      GT) between device events, and the share of the whole rows-form call that is not these stages.
  (d) optionally the headline lines of bench.py runs on the parent commit's library and on this tree's, alternating on the same box
      (--bench-parent / --bench-this: files holding one JSON line per run), copied in side by side.

    python tools/sw05_select.py [--items 65536] [--runs 5] [--commit ID] [--out profiles/sw05_select.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--commit")
    ap.add_argument("--bench-parent")
    ap.add_argument("--bench-this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sw05_select.json"))
    args = ap.parse_args()
    import torch
    from sw05_fixture import Instance, at_size_attributes
    from gopairingbasedcryptography_amd import _build, bn254 as eng, sw05
    _build.build_library()
    eng.init(0)
    dev = torch.device("cuda", 0)
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None

    def timed(fn, runs=args.runs, warmup=1):
        out = None
        for _ in range(warmup):
            out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), ms, out

    def wall(fn, runs=args.runs, warmup=1):
        out = None
        for _ in range(warmup):
            out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(runs):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms), ms, out

    doc = {"what": "fr_find_common and SW05 decryption from attribute rows (sw05.decrypt_batch / decrypt_batch_large), one MI355X",
           "device": torch.cuda.get_device_name(0), "commit": commit, "date": time.strftime("%Y-%m-%d"), "runs": args.runs,
           "timing": "median of the runs after one warm-up: device events on the stream for kernels and stages, wall clock with a device synchronisation for whole calls"}
    n, a, n_key, d = args.items, 24, 32, 16
    key_attrs, cts = at_size_attributes(n, a, n_key, d, every=64)
    t0 = time.perf_counter()
    ct_rows_host = sw05.attribute_rows(cts)
    t_rows = time.perf_counter() - t0
    ct_rows, key_rows = torch.from_numpy(ct_rows_host).to(dev), torch.from_numpy(sw05.attribute_rows(key_attrs)).to(dev)
    # ---- (a) the kernel alone
    rng = np.random.default_rng(2005)
    rand = lambda rows: torch.from_numpy(rng.integers(0, 256, size=rows * 32, dtype=np.uint8)).to(dev)
    shapes = []
    big_m = 256
    pool = rand(2 * big_m)                                                      # lists drawn from twice the set: about half of an item's list is held
    pick = torch.from_numpy(rng.integers(0, 2 * big_m, size=(1 << 12) * 256)).to(dev)
    for label, S, L, k, m, aa, dd in (("2^16 x (24, 32, 16), one set", key_rows.reshape(-1), ct_rows.reshape(-1), n, n_key, a, d),
                                      ("2^16 x (24, 32, 16), a set per item", key_rows.reshape(1, -1).expand(n, n_key * 32).contiguous().reshape(-1), ct_rows.reshape(-1), n, n_key, a, d),
                                      ("2^12 x (256, 256, 128), one set", pool.reshape(-1, 32)[:big_m].contiguous().reshape(-1), pool.reshape(-1, 32)[pick].reshape(-1), 1 << 12, big_m, 256, 128)):
        outs = [torch.empty(k * dd * 4, dtype=torch.uint8, device=dev), torch.empty(k * dd * 4, dtype=torch.uint8, device=dev), torch.empty(k * dd * 32, dtype=torch.uint8, device=dev),
                torch.empty(k, dtype=torch.uint8, device=dev)]
        t, smp, res = timed(lambda: eng.fr_find_common(S, L, m, aa, dd, *outs))
        shapes.append({"shape": label, "items": k, "m": m, "a": aa, "d": dd, "ms": t, "samples_ms": smp, "items_per_s": k / (t * 1e-3), "ok": int(res[3].sum())})
    doc["fr_find_common"] = shapes
    # ---- (b), (c) the two decrypts in both forms
    doc["shape"] = {"ciphertexts": n, "attributes_per_ciphertext": a, "key_attributes": n_key, "d": d, "below_threshold": n // 64,
                    "attribute_rows_of_the_ciphertexts_s": t_rows}
    for large in (False, True):
        name = "decrypt_batch_large" if large else "decrypt_batch"
        inst = Instance(eng, d, key_attrs, cts, n_univ=a if large else None, dev=dev, tag="m")
        key_dev = (key_rows,) + tuple(torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in inst.key[1:])
        if large:
            ints = lambda i=inst: sw05.decrypt_batch_large(eng, i.key, d, cts, i.E, i.e_pp, i.e_prime)
            rows = lambda i=inst, kd=key_dev: sw05.decrypt_batch_large(eng, kd, d, ct_rows, i.E, i.e_pp, i.e_prime)
        else:
            ints = lambda i=inst: sw05.decrypt_batch(eng, i.key, d, cts, i.E, i.e_prime)
            rows = lambda i=inst, kd=key_dev: sw05.decrypt_batch(eng, kd, d, ct_rows, i.E, i.e_prime)
        t_int, s_int, (m_int, ok_int) = wall(ints)
        t_row, s_row, (m_row, ok_row) = wall(rows)
        same = bool(torch.equal(m_int, m_row)) and bool(torch.equal(ok_int, ok_row))
        good = ok_row.bool()
        assert same and int((~good).sum()) == n // 64 and bool((m_row[good] == inst.msgs.reshape(n, 384)[good]).all()), name
        p = sw05._RowsPlan(eng, key_dev[0], d, ct_rows, inst.E, inst.e_prime)
        t_sel, _, sel = timed(lambda: eng.fr_find_common(key_rows.reshape(-1), ct_rows.reshape(-1), n_key, a, d))
        sets = sel[2].reshape(n, d * 32)[torch.from_numpy(p.good).to(dev)].contiguous().reshape(-1)
        t_lag, _, delta = timed(lambda: eng.fr_lagrange_basis(sets, d))
        delta = delta.reshape(p.ng, d, 32)
        if large:
            epp = p.rows(inst.e_pp.reshape(n, 64)).reshape(p.ng, 1, 64).expand(p.ng, d, 64)
            bases = torch.cat([p.key_rows(key_dev[1], 64), epp], 1).contiguous().reshape(-1)
            neg = lambda: torch.cat([delta, eng.fr_neg(delta.reshape(-1)).reshape(p.ng, d, 32)], 1).contiguous().reshape(-1)
            t_smul, _, P = timed(lambda: eng.g1_scalar_mul(bases, neg()))
            Q = torch.cat([p.ct_rows(), p.key_rows(key_dev[2], 128)], 1).contiguous().reshape(-1)
            pairs = 2 * d
        else:
            bases = p.key_rows(key_dev[1], 64).contiguous().reshape(-1)
            t_smul, _, P = timed(lambda: eng.g1_scalar_mul(bases, delta.reshape(-1)))
            Q = p.ct_rows().contiguous().reshape(-1)
            pairs = d
        t_pair, _, den = timed(lambda: eng.multi_pair(P.reshape(-1), Q, p.seg(pairs)))
        ep = p.rows(p.e_prime)
        t_gt, _, _ = timed(lambda: (eng.gt_mul if large else eng.gt_div)(ep, den))
        t_plan, s_plan, _ = wall(lambda: sw05._RowsPlan(eng, key_dev[0], d, ct_rows, inst.E, inst.e_prime))
        stages = t_sel + t_lag + t_smul + t_pair + t_gt
        doc[name] = {"integer_form_ms": t_int, "integer_form_samples_ms": s_int, "rows_form_ms": t_row, "rows_form_samples_ms": s_row, "ratio": t_int / t_row,
                     "messages_and_ok_equal": same, "ciphertexts_per_s_rows_form": n / (t_row * 1e-3),
                     "stages_ms": {"find_common": t_sel, "lagrange": t_lag, "scalar_mul": t_smul, "multi_pair": t_pair, "gt": t_gt, "sum": stages},
                     "rows_form_not_in_stages_ms": t_row - stages, "rows_form_share_not_in_stages": (t_row - stages) / t_row,
                     "rows_plan_alone_ms": t_plan, "rows_plan_alone_samples_ms": s_plan,
                     "rows_plan_alone_is": "selection, the one wait for ok, the gather of the Lagrange sets and fr_lagrange_basis, by the wall clock"}
        del inst
        eng.release_workspaces()
    for key, path in (("bench_py_parent", args.bench_parent), ("bench_py_this", args.bench_this)):
        if path and os.path.exists(path):
            runs = [json.loads(ln) for ln in open(path).read().splitlines() if ln.startswith("{")]
            doc[key] = [{f: r.get(f) for f in ("metric", "value", "unit", "steps", "warmup", "ms_per_step")} for r in runs]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
