#!/usr/bin/env python3
"""Threshold-tree forests measured on one MI355X, in one process: writes profiles/share_forest.json.

  (1) the cost of generality: ITEMS items over ONE tree — 256-of-256, 128-of-256, 16 x (16-of-16) under 16-of-16, and two trees whose
      levels are no power of two wide, 2-of-3 and 3-of-5 over five 2-of-3 gates — through ShareTree and through a ShareForest of that
      one tree, share and weights, on the same HBM-resident inputs; the bytes must be equal; the ratio is reported, not gated;
  (2) the mixed call: ITEMS items over 16 and over 256 distinct flat policies t-of-n, n in 16 .. 256, assigned at random.  ShareForest.share
      / .weights against the single-policy route: group by policy on the host, one ShareTree per policy (made beforehand; the time to make
      them is reported beside it), gather, call, scatter back into the padded rows.  The bytes must be equal.  Then
      bsw07.encrypt_batch_policies against per-policy bsw07.encrypt_batch, and bsw07.decrypt_batch_policies against per-policy
      bsw07.decrypt_batch_keys, whole calls by the wall clock with a device synchronisation, the two routes alternating.  The key
      components of the decryption are arbitrary G2 points (the same for every item): the routes are compared with each other, not with
      the messages;
  (3) optionally the headline lines of bench.py runs on the parent commit's library and on this tree's (--bench-parent / --bench-this:
      files holding one JSON line per run, in the order they were run), copied in side by side.

    python tools/bench_share_forest.py [--runs 5] [--items 65536] [--planner-items 65536] [--commit ID] [--out profiles/share_forest.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402


def stats(ms):
    return {"min_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "all_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5, help="calls back to back inside one timed window of a device entry")
    ap.add_argument("--items", type=int, default=1 << 16)
    ap.add_argument("--planner-items", type=int, default=1 << 16, help="ciphertexts of the Encrypt / Decrypt comparison; 0 skips it")
    ap.add_argument("--policies", type=int, nargs="*", default=[16, 256])
    ap.add_argument("--commit")
    ap.add_argument("--bench-parent")
    ap.add_argument("--bench-this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "share_forest.json"))
    args = ap.parse_args()
    import torch
    from gopairingbasedcryptography_amd import _build, bn254 as eng, bsw07
    _build.build_library()
    eng.init(0)
    dev = torch.device("cuda", 0)
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
    k = args.items
    doc = {"what": "ShareForest (a threshold tree per item) beside ShareTree (one tree per call), and the BSW07 planners over both, one MI355X",
           "device": torch.cuda.get_device_name(0), "commit": commit, "date": time.strftime("%Y-%m-%d"), "runs": args.runs, "reps": args.reps, "items": k,
           "timing": "every shape warmed up once; device entries: `runs` repetitions, each `reps` calls back to back between two device events, over reps; grouped "
                     "routes and whole planner calls: wall clock with a device synchronisation, the routes alternating; min, median and max"}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / args.reps)
        return stats(ms)

    def alternating(legs, runs):
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in legs}
        for _ in range(runs):
            for name, fn in legs.items():
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3)
        return {name: stats(v) for name, v in ms.items()}

    nprng = np.random.default_rng(2007)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rand = lambda *shape: put(nprng.integers(0, 256, size=shape + (32,), dtype=np.uint8))
    ids_of = lambda a: put(np.ascontiguousarray(a, dtype=np.uint32).view(np.uint8)).view(torch.int32)
    Leaf, Threshold = bsw07.Leaf, bsw07.Threshold
    flat = lambda t, n: Threshold(t, *[Leaf(a) for a in range(n)])

    # ---- (1) one tree: the forest of it beside ShareTree
    doc["one_tree"] = []
    # the last two have levels that are no power of two (3; 5 and 15): the forest's fixed lanes per item leave part of a wave idle there
    for name, tree in (("256-of-256", flat(256, 256)), ("128-of-256", flat(128, 256)), ("16x(16-of-16)", Threshold(16, *[flat(16, 16) for _ in range(16)])),
                       ("2-of-3", flat(2, 3)), ("3-of-5 over 5x(2-of-3)", Threshold(3, *[flat(2, 3) for _ in range(5)]))):
        nodes, _ = bsw07.share_plan(tree)
        t, f = eng.ShareTree(nodes), eng.ShareForest([nodes])
        L, C = t.leaves, t.coeffs
        secrets, coeffs, held = rand(k).reshape(-1), rand(k, C).reshape(-1), torch.ones(k * L, dtype=torch.uint8, device=dev)
        ids = torch.zeros(k, dtype=torch.int32, device=dev)
        out_t, out_f = (torch.empty(k * L * 32, dtype=torch.uint8, device=dev) for _ in range(2))
        ok_t, ok_f, ok_s = (torch.empty(k, dtype=torch.uint8, device=dev) for _ in range(3))
        rec = {"tree": name, "items": k, "leaves": L, "coeffs": C}
        rec["share_tree"] = timed(lambda: t.share(secrets, coeffs, out=out_t))
        rec["share_forest"] = timed(lambda: f.share(ids, secrets, coeffs, out=out_f, ok_out=ok_s))
        rec["share_bytes_equal"] = bool(torch.equal(out_t, out_f))
        rec["tree_weights"] = timed(lambda: t.weights(held, out=out_t, ok_out=ok_t))
        rec["forest_weights"] = timed(lambda: f.weights(ids, held, out=out_f, ok_out=ok_f))
        rec["weights_bytes_equal"] = bool(torch.equal(out_t, out_f) and torch.equal(ok_t, ok_f))
        rec["share_forest_over_tree"] = rec["share_forest"]["median_ms"] / rec["share_tree"]["median_ms"]
        rec["weights_forest_over_tree"] = rec["forest_weights"]["median_ms"] / rec["tree_weights"]["median_ms"]
        doc["one_tree"].append(rec)
        print("%s x %d: share %.3f ms tree / %.3f ms forest (%.2f x), weights %.3f / %.3f ms (%.2f x), bytes equal %s %s" % (
            name, k, rec["share_tree"]["median_ms"], rec["share_forest"]["median_ms"], rec["share_forest_over_tree"], rec["tree_weights"]["median_ms"],
            rec["forest_weights"]["median_ms"], rec["weights_forest_over_tree"], rec["share_bytes_equal"], rec["weights_bytes_equal"]), flush=True)
        t.close()
        f.close()
        del secrets, coeffs, held, out_t, out_f
        torch.cuda.empty_cache()
        save()

    # ---- (2) many policies in one call
    doc["mixed"] = []
    for T in args.policies:
        shapes = set()
        while len(shapes) < T:
            n = int(nprng.integers(16, 257))
            shapes.add((int(nprng.integers(1, n + 1)), n))
        shapes = sorted(shapes, key=lambda s: (s[1], s[0]))
        trees = [flat(t, n) for t, n in shapes]
        plan = bsw07.forest_plan(trees)
        node_lists = [nodes for nodes, _ in plan[0]]
        Lmax, Cmax = max(n for _, n in shapes), max(t - 1 for t, _ in shapes)
        policy = nprng.integers(0, T, size=k).astype(np.uint32)
        groups = [np.nonzero(policy == t)[0] for t in range(T)]
        t0 = time.perf_counter()
        forest = eng.ShareForest(node_lists)
        forest_create_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        handles = [eng.ShareTree(nodes) for nodes in node_lists]
        trees_create_ms = (time.perf_counter() - t0) * 1e3
        ids = ids_of(policy)
        secrets, coeffs = rand(k), rand(k, Cmax) if Cmax else None
        held = put((nprng.random((k, Lmax)) < 0.9).astype(np.uint8))
        gidx = [put(g.astype(np.int64)) for g in groups]
        out_f, ok_f = torch.empty((k, Lmax, 32), dtype=torch.uint8, device=dev), torch.empty(k, dtype=torch.uint8, device=dev)

        def grouped_share():
            out = torch.zeros((k, Lmax, 32), dtype=torch.uint8, device=dev)
            for h, g in zip(handles, gidx):
                if len(g):
                    q = coeffs.index_select(0, g)[:, :h.coeffs].contiguous().reshape(-1) if h.coeffs else None
                    out[g, :h.leaves] = h.share(secrets.index_select(0, g).reshape(-1), q)
            return out

        def grouped_weights():
            w, ok = torch.zeros((k, Lmax, 32), dtype=torch.uint8, device=dev), torch.zeros(k, dtype=torch.uint8, device=dev)
            for h, g in zip(handles, gidx):
                if len(g):
                    wi, oki = h.weights(held.index_select(0, g)[:, :h.leaves].contiguous().reshape(-1))
                    w[g, :h.leaves], ok[g] = wi, oki
            return w, ok
        rec = {"policies": T, "items": k, "leaves": [min(n for _, n in shapes), Lmax], "Cmax": Cmax, "forest_create_ms": forest_create_ms, "share_trees_create_ms": trees_create_ms}
        rec["share_forest_events"] = timed(lambda: forest.share(ids, secrets.reshape(-1), coeffs.reshape(-1) if Cmax else None, out=out_f, ok_out=ok_f))
        rec.update(alternating({"share_forest": lambda: forest.share(ids, secrets.reshape(-1), coeffs.reshape(-1) if Cmax else None, out=out_f, ok_out=ok_f),
                                "share_grouped": grouped_share}, args.runs))
        rec["share_bytes_equal"] = bool(torch.equal(grouped_share(), out_f))
        rec["forest_weights_events"] = timed(lambda: forest.weights(ids, held.reshape(-1), out=out_f, ok_out=ok_f))
        rec.update(alternating({"forest_weights": lambda: forest.weights(ids, held.reshape(-1), out=out_f, ok_out=ok_f), "weights_grouped": grouped_weights}, args.runs))
        gw, gok = grouped_weights()
        rec["weights_bytes_equal"] = bool(torch.equal(gw, out_f) and torch.equal(gok, ok_f))
        rec["satisfied"] = int(ok_f.sum().item())
        rec["share_grouped_over_forest"] = rec["share_grouped"]["median_ms"] / rec["share_forest"]["median_ms"]
        rec["weights_grouped_over_forest"] = rec["weights_grouped"]["median_ms"] / rec["forest_weights"]["median_ms"]
        print("%d policies x %d: share %.3f ms forest / %.3f ms grouped (%.2f x), weights %.3f / %.3f ms (%.2f x), bytes equal %s %s" % (
            T, k, rec["share_forest"]["median_ms"], rec["share_grouped"]["median_ms"], rec["share_grouped_over_forest"], rec["forest_weights"]["median_ms"],
            rec["weights_grouped"]["median_ms"], rec["weights_grouped_over_forest"], rec["share_bytes_equal"], rec["weights_bytes_equal"]), flush=True)
        for h in handles:
            h.close()
        forest.close()
        del secrets, coeffs, held, out_f, ok_f, gw, gok
        torch.cuda.empty_cache()
        doc["mixed"].append(rec)
        save()

        # ---- the planners over the same policies
        n = args.planner_items
        if not n:
            continue
        pol = policy[:n] if n <= k else nprng.integers(0, T, size=n).astype(np.uint32)
        rows = [np.nonzero(pol == t)[0] for t in range(T)]
        ridx = [put(r.astype(np.int64)) for r in rows]
        g1, g2 = (put(x) for x in eng.generators())
        e = eng.pair_batch(g1, g2)
        e_alpha = eng.gt_exp(e.reshape(-1), rand(1).reshape(-1)).reshape(-1)
        hpk = eng.g1_scalar_mul(g1, rand(1).reshape(-1)).reshape(-1)
        H1 = eng.g1_scalar_mul_base(rand(Lmax).reshape(-1)).reshape(Lmax, 64).cpu().numpy()
        h1 = {a: H1[a] for a in range(Lmax)}
        messages = eng.gt_exp(e.expand(n, 384).contiguous().reshape(-1), rand(n).reshape(-1)).reshape(n, 384)
        s, coeffs = rand(n), rand(n, Cmax) if Cmax else None
        pids = ids_of(pol)
        pr = {"ciphertexts": n}

        def per_policy_encrypt(tables):
            c_tilde, c = torch.zeros((n, 384), dtype=torch.uint8, device=dev), torch.zeros((n, 64), dtype=torch.uint8, device=dev)
            cy, cyp = torch.zeros((n, Lmax, 64), dtype=torch.uint8, device=dev), torch.zeros((n, Lmax, 64), dtype=torch.uint8, device=dev)
            for t, g in enumerate(ridx):
                if len(g):
                    C_t, L_t = shapes[t][0] - 1, shapes[t][1]
                    q = coeffs.index_select(0, g)[:, :C_t].contiguous() if C_t else None
                    a, b, y, yp = bsw07.encrypt_batch(eng, plan[0][t], hpk, e_alpha, h1, messages.index_select(0, g), s.index_select(0, g), q, tables=tables)
                    c_tilde[g], c[g], cy[g, :L_t], cyp[g, :L_t] = a, b, y, yp
            return c_tilde, c, cy, cyp
        for tables in (False, True):
            tag = "tables" if tables else "var_base"
            res = alternating({"encrypt_batch_policies_" + tag: lambda: bsw07.encrypt_batch_policies(eng, plan, pids, hpk, e_alpha, h1, messages, s, coeffs, tables=tables),
                               "encrypt_per_policy_" + tag: lambda: per_policy_encrypt(tables)}, max(2, args.runs // 2))
            pr.update(res)
            ct = bsw07.encrypt_batch_policies(eng, plan, pids, hpk, e_alpha, h1, messages, s, coeffs, tables=tables)
            pr["encrypt_bytes_equal_" + tag] = bool(all(torch.equal(a, b) for a, b in zip(ct, per_policy_encrypt(tables))))
            pr["encrypt_per_policy_over_policies_" + tag] = res["encrypt_per_policy_" + tag]["median_ms"] / res["encrypt_batch_policies_" + tag]["median_ms"]
            print("  %d ciphertexts, %s: encrypt_batch_policies %.1f ms, per policy %.1f ms, bytes equal %s" % (
                n, tag, res["encrypt_batch_policies_" + tag]["median_ms"], res["encrypt_per_policy_" + tag]["median_ms"], pr["encrypt_bytes_equal_" + tag]), flush=True)
            save()
        c_tilde, c, cy, cyp = ct
        keys = eng.g2_scalar_mul_base(rand(2 * Lmax + 1).reshape(-1)).reshape(2 * Lmax + 1, 128)
        dj, djp, d_key = keys[:Lmax].expand(n, Lmax, 128).contiguous(), keys[Lmax:2 * Lmax].expand(n, Lmax, 128).contiguous(), keys[2 * Lmax].cpu().numpy()
        held = put((nprng.random((n, Lmax)) < 0.9).astype(np.uint8))

        def per_policy_decrypt():
            msgs, ok = torch.zeros((n, 384), dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
            for t, g in enumerate(ridx):
                if len(g):
                    L_t = shapes[t][1]
                    cut = lambda a: a.index_select(0, g)[:, :L_t].contiguous()
                    m, o = bsw07.decrypt_batch_keys(eng, plan[0][t], cut(held), d_key, cut(dj), cut(djp), c_tilde.index_select(0, g), c.index_select(0, g), cut(cy), cut(cyp))
                    msgs[g], ok[g] = m, o
            return msgs, ok
        policies_decrypt = lambda: bsw07.decrypt_batch_policies(eng, plan, pids, held, d_key, dj, djp, c_tilde, c, cy, cyp)
        res = alternating({"decrypt_batch_policies": policies_decrypt, "decrypt_per_policy": per_policy_decrypt}, max(2, args.runs // 2))
        pr.update(res)
        (m1, o1), (m2, o2) = policies_decrypt(), per_policy_decrypt()
        pr["decrypt_bytes_equal"] = bool(torch.equal(m1, m2) and torch.equal(o1, o2))
        pr["decrypt_satisfied"] = int(o1.sum().item())
        pr["decrypt_per_policy_over_policies"] = res["decrypt_per_policy"]["median_ms"] / res["decrypt_batch_policies"]["median_ms"]
        print("  %d ciphertexts: decrypt_batch_policies %.1f ms, per policy %.1f ms, bytes equal %s, %d satisfied" % (
            n, res["decrypt_batch_policies"]["median_ms"], res["decrypt_per_policy"]["median_ms"], pr["decrypt_bytes_equal"], pr["decrypt_satisfied"]), flush=True)
        rec["planners"] = pr
        del messages, s, coeffs, ct, c_tilde, c, cy, cyp, dj, djp, held, m1, m2
        torch.cuda.empty_cache()
        save()
    for name, path in (("bench_py_parent", args.bench_parent), ("bench_py_this", args.bench_this)):
        if path and os.path.exists(path):
            runs = [json.loads(ln) for ln in open(path).read().splitlines() if ln.startswith("{")]
            doc[name] = [{f: r.get(f) for f in ("metric", "value", "unit", "steps", "warmup", "ms_per_step")} for r in runs]
    save()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
