#!/usr/bin/env python3
"""LSSS matrices from formulas and the 0 / 1 decryption route measured on one MI355X, in one process, the routes alternating on the same
inputs: writes profiles/formula_policies.json.

  (1) fr_lsss_from_formula on HBM-resident codes at 2^14 formulas x 31 nodes (rows = cols = 16) and 2^12 x 127 nodes (64 x 64): median of
      RUNS of REPS calls back to back between two device events, and the bytes written over that time as a fraction of the HBM peak (the kernel has no other bound);
      beside it the route without the entry: waters11.pad_policies over the same policies as distinct (matrix, rho) pairs plus the upload of
      its block, by the wall clock (on --parent-policies of them; the per-policy time is what compares);
  (2) formula_select on those codes and random masks, beside fr_lsss_weights on the built matrices and the same masks;
  (3) waters11.decrypt_batch_formulas against decrypt_batch and decrypt_batch(msm=True) on 2^14 ciphertexts under 16-leaf formulas, whole
      calls by the wall clock, synchronised; the messages and ok of the three are compared;
  (4) optionally the headline lines of bench.py runs on the parent commit's library and on this tree's (--bench-parent / --bench-this: files
      holding one JSON line per run), copied in side by side.

    python tools/formula_policies.py [--runs 5] [--commit ID] [--out profiles/formula_policies.json]
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

HBM_PEAK_BYTES_PER_S = 8.0e12          # MI355X: 8 TB/s


def random_formula(n, rng, attrs):
    if n == 1:
        return int(rng.integers(0, attrs))
    i = int(rng.integers(1, n))
    return ("and" if rng.integers(0, 2) else "or", random_formula(i, rng, attrs), random_formula(n - i, rng, attrs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--ciphertexts", type=int, default=1 << 14, help="0: the single entries only")
    ap.add_argument("--parent-policies", type=int, default=1024)
    ap.add_argument("--commit")
    ap.add_argument("--bench-parent")
    ap.add_argument("--bench-this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "formula_policies.json"))
    args = ap.parse_args()
    import torch
    import bn254_py as o
    from gopairingbasedcryptography_amd import _build, bn254 as eng, formula, waters11
    _build.build_library()
    eng.init(0)
    dev = torch.device("cuda", 0)
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None

    def timed(fn, runs=args.runs, warmup=1, reps=args.reps):
        """ms per call: `reps` calls back to back between two device events (one call alone is a window that measures the clock)"""
        out = None
        for _ in range(warmup):
            out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                out = fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / reps)
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

    doc = {"what": "fr_lsss_from_formula, formula_select and waters11.decrypt_batch_formulas beside the routes without them, one MI355X",
           "device": torch.cuda.get_device_name(0), "commit": commit, "date": time.strftime("%Y-%m-%d"), "runs": args.runs,
           "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
           "reps": args.reps,
           "timing": "median of the runs after one warm-up: for single entries the time between two device events around `reps` calls back to back, over reps; "
                     "wall clock with a device synchronisation for whole calls and host routes"}
    rng = np.random.default_rng(2011)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    # ---- (1), (2) the two entries alone
    build, select = [], []
    for k, leaves, R in ((1 << 14, 16, 16), (1 << 12, 64, 64)):
        pool = [random_formula(leaves, rng, 48) for _ in range(256)]
        trees = [pool[j % len(pool)] for j in range(k)]
        nodes_host = formula.encode(trees)
        nodes = to_dev(nodes_host)
        outs = [torch.empty(k * R * R * 32, dtype=torch.uint8, device=dev), torch.empty(k * R * 8, dtype=torch.uint8, device=dev),
                torch.empty(k * 8, dtype=torch.uint8, device=dev), torch.empty(k, dtype=torch.uint8, device=dev)]
        t, smp, res = timed(lambda: eng.fr_lsss_from_formula(nodes, R, R, *outs))
        written = k * (R * R * 32 + R * 8 + 8 + 1)
        m = min(k, args.parent_policies)
        policies = [tuple(list(x) for x in formula.lsss_matrix(pool[j % len(pool)])) for j in range(m)]          # distinct objects: each is converted
        t_pad, s_pad, block = wall(lambda: to_dev(waters11.pad_policies(policies, R, R).matrix), runs=min(args.runs, 3), warmup=0)
        same = bool(torch.equal(block, res[0][:m]))
        build.append({"formulas": k, "nodes": int(nodes_host.shape[1]), "rows": R, "cols": R, "ms": t, "samples_ms": smp, "bytes_written": written,
                      "bytes_per_s": written / (t * 1e-3), "fraction_of_hbm_peak": written / (t * 1e-3) / HBM_PEAK_BYTES_PER_S, "ok": int(res[3].sum()),
                      "pad_policies_and_upload": {"policies": m, "ms": t_pad, "samples_ms": s_pad, "ms_per_policy": t_pad / m, "same_bytes_as_the_device_matrices": same},
                      "from_formula_ms_per_policy": t / k})
        held = to_dev((rng.integers(0, 4, (k, R)) > 0).astype(np.uint8))
        t_sel, s_sel, sel = timed(lambda: eng.formula_select(nodes, held.reshape(-1), R))
        t_w, s_w, solved = timed(lambda: eng.fr_lsss_weights(res[0].reshape(-1), R, R, held.reshape(-1)))
        select.append({"formulas": k, "rows": R, "formula_select_ms": t_sel, "formula_select_samples_ms": s_sel, "fr_lsss_weights_ms": t_w, "fr_lsss_weights_samples_ms": s_w,
                       "ratio": t_w / t_sel, "ok_equal": bool(torch.equal(sel[1], solved[1])), "ok": int(sel[1].sum())})
        del outs, res, block, solved, nodes, held
    doc["fr_lsss_from_formula"], doc["formula_select"] = build, select
    # ---- (3) the three decryption routes
    n, leaves = args.ciphertexts, 16
    if not n:
        print(json.dumps(doc, indent=1))
        return
    universe = list(range(100, 148))
    key_attrs = [u for u in universe if u % 3]
    sc = lambda tag, i=0: o.bench_scalar("fp-" + tag, i)
    pool = [random_formula(leaves, rng, len(universe)) for _ in range(64)]
    relabel = lambda t: universe[t] if not isinstance(t, tuple) else (t[0], relabel(t[1]), relabel(t[2]))
    pool = [relabel(t) for t in pool]
    nodes_host = formula.encode([pool[j % len(pool)] for j in range(n)])
    nodes = to_dev(nodes_host)
    g1, g2 = eng.generators()
    e = np.asarray(eng.pair_batch(g1, g2)).reshape(1, 384)
    alpha, a, t = sc("alpha"), sc("a"), sc("t")
    tau = {u: sc("tau", u) for u in universe}
    g1a = np.asarray(eng.g1_scalar_mul_base([a])).reshape(64)
    e_alpha = np.asarray(eng.gt_exp(e, [alpha])).reshape(384)
    hs = np.asarray(eng.g1_scalar_mul_base([tau[u] for u in universe])).reshape(-1, 64)
    kl = np.asarray(eng.g1_scalar_mul_base([(alpha + a * t) % o.R] + [tau[u] * t % o.R for u in key_attrs])).reshape(-1, 64)
    key = (kl[0].copy(), np.asarray(eng.g2_scalar_mul_base([t])).reshape(128), {u: kl[1 + i].copy() for i, u in enumerate(key_attrs)})
    rand = lambda rows: torch.from_numpy(rng.integers(0, 256, size=rows * 32, dtype=np.uint8)).to(dev)
    msgs = eng.gt_exp(to_dev(np.tile(e, (n, 1))), rand(n))
    pad = formula.padded(eng, nodes, like=msgs)
    ct = waters11.encrypt_batch(eng, g1a, e_alpha, {u: hs[i] for i, u in enumerate(universe)}, pad, msgs, rand(n), rand(n * (pad.cols - 1)), rand(n * pad.rows))
    torch.cuda.synchronize()
    routes = {"decrypt_batch_formulas": lambda: waters11.decrypt_batch_formulas(eng, key, nodes, *ct),
              "decrypt_batch": lambda: waters11.decrypt_batch(eng, key, pad, *ct),
              "decrypt_batch_msm": lambda: waters11.decrypt_batch(eng, key, pad, *ct, msm=True)}
    samples = {name: [] for name in routes}
    results = {name: fn() for name, fn in routes.items()}                         # the warm-up, and what is compared
    torch.cuda.synchronize()
    for _ in range(args.runs):                                                    # the routes alternate on the same inputs
        for name, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            samples[name].append((time.perf_counter() - t0) * 1e3)
    ref_m, ref_ok = results["decrypt_batch"]
    good = ref_ok.bool()
    doc["waters11_decrypt"] = {
        "ciphertexts": n, "rows": pad.rows, "cols": pad.cols, "satisfied": int(good.sum()),
        "satisfied_return_the_plaintext": bool((ref_m[good] == msgs.reshape(n, 384)[good]).all()),
        "messages_and_ok_equal": all(bool(torch.equal(m, ref_m)) and bool(torch.equal(k_, ref_ok)) for m, k_ in results.values()),
        "ms": {name: statistics.median(v) for name, v in samples.items()}, "samples_ms": samples,
        "decrypt_batch_over_formulas": statistics.median(samples["decrypt_batch"]) / statistics.median(samples["decrypt_batch_formulas"]),
        "decrypt_batch_msm_over_formulas": statistics.median(samples["decrypt_batch_msm"]) / statistics.median(samples["decrypt_batch_formulas"])}
    for name, path in (("bench_py_parent", args.bench_parent), ("bench_py_this", args.bench_this)):
        if path and os.path.exists(path):
            runs = [json.loads(ln) for ln in open(path).read().splitlines() if ln.startswith("{")]
            doc[name] = [{f: r.get(f) for f in ("metric", "value", "unit", "steps", "warmup", "ms_per_step")} for r in runs]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
