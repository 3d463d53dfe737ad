#!/usr/bin/env python3
"""The fixed-base GT tables measured on one MI355X: ONE step per invocation, merged into profiles/gt_fixed_base.json (run every step
under a time limit of its own).

  --step kernel    GTFixedBase.indexed at 2^16 and 2^20 HBM-resident exponents beside the routes it replaces, in the same run:
                       terms = 1   table.pow(k)                          |  gt_exp on the base replicated n times (the parent's path)
                       terms = 2   table.indexed over one shared row     |  two gt_exp + gt_mul;  gt_multi_exp over two-factor segments
                   and beside a plain device copy of the bytes the call writes — the rate a kernel that computes nothing gets.  The
                   outputs of the routes are compared first.  Also the table build for 1 and 16 bases (wall clock: create, build, wait).
  --step waters05  waters05.encrypt_batch at 2^16 items with and without gt_table
  --step gentry06  gentry06.encrypt_batch at 2^16 items, CPA (k = 1) and CCA (k = 3), each with and without gt_table
  --step bb04sibe  bb04sibe keygen / encrypt / decrypt at 2^16 items (a key per ciphertext, and one key for all)
  --step bb04ibe   bb04ibe keygen / encrypt / decrypt at 2^12 items and identity length 256, with the time per engine entry inside
                   each call (every entry between two device synchronisations: the split adds up to more than the whole call's time)

Whole-call device times: after a warm-up, `runs` repetitions of `reps` calls between two device events, the legs of a comparison
alternating.  Planner calls: wall clock around a device synchronisation.  Not measured: host-pointer entries, more than one device.

    python tools/gt_fixed_base_bench.py --step kernel [--runs 5] [--reps 3] [--out profiles/gt_fixed_base.json]
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

SEED = bytes(range(11, 43))


def stats(ms):
    return {"min_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "all_ms": ms}


class Split:
    """an engine (or a table) whose every call runs between two device synchronisations; ms[name] collects the times"""

    def __init__(self, target, torch, ms, prefix=""):
        self._target, self._torch, self._ms, self._prefix = target, torch, ms, prefix

    def __getattr__(self, name):
        fn = getattr(self._target, name)
        if not callable(fn):
            return fn

        def timed(*a, **kw):
            self._torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn(*a, **kw)
            self._torch.cuda.synchronize()
            self._ms.setdefault(self._prefix + name, []).append((time.perf_counter() - t0) * 1e3)
            return res
        return timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=["kernel", "waters05", "gentry06", "bb04sibe", "bb04ibe"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="calls back to back inside one timed window")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--items", type=int, default=1 << 16)
    ap.add_argument("--ibe-items", type=int, default=1 << 12)
    ap.add_argument("--planner-runs", type=int, default=3)
    ap.add_argument("--commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_fixed_base.json"))
    args = ap.parse_args()
    import torch
    from gopairingbasedcryptography_amd import _build, bb04ibe, bb04sibe, bn254 as eng, gentry06, waters05
    _build.build_library()
    eng.init(0)
    dev = torch.device("cuda", 0)
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc.update({"what": "fixed-base GT tables (GTFixedBase.pow / indexed) beside gt_exp on a replicated base, gt_multi_exp and a plain copy; the Encrypt "
                        "planners with and without gt_table; the BB04 planners; one MI355X, one run",
                "device": torch.cuda.get_device_name(0), "commit": commit, "date": time.strftime("%Y-%m-%d"),
                "timing": "kernels: warm-up, then `runs` repetitions of `reps` calls between two device events, legs alternating; planner calls and the "
                          "table build: wall clock around a device synchronisation",
                "not_measured": ["the host-pointer entries", "more than one device", "LW11, BSW07 and AFP25 Encrypt with a table"]})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    def timed(legs):
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in legs}
        for _ in range(args.runs):
            for name, fn in legs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.reps):
                    fn()
                b.record()
                b.synchronize()
                ms[name].append(a.elapsed_time(b) / args.reps)
        return {name: stats(v) for name, v in ms.items()}

    def wall(fn, runs=None):
        fn()
        ms = []
        for _ in range(runs or args.planner_runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return stats(ms)

    like = torch.empty(0, dtype=torch.uint8, device=dev)
    scalars = lambda k, stream=3: eng.fr_random(SEED, k, stream=stream, like=like)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    g1, g2 = eng.generators()
    e = put(eng.pair_batch(g1, g2)).reshape(1, 384)
    rep = lambda x, n: x.reshape(1, 384).expand(n, 384).contiguous()
    same = lambda a, b: bool((a.reshape(-1) == b.reshape(-1)).all())

    def planner_legs(name, items, legs, check):
        out = doc[name] = {"items": items, "planner_runs": args.planner_runs, "calls": {}}
        assert check()
        for leg, fn in legs.items():
            out["calls"][leg] = wall(fn)
            print("%s %s: %.2f ms" % (name, leg, out["calls"][leg]["median_ms"]), flush=True)
            save()
        return out

    if args.step == "kernel":
        two = torch.cat([e, eng.gt_exp(e, [7]).reshape(1, 384)])
        t1, t2 = eng.GTFixedBase(e), eng.GTFixedBase(two)
        row = torch.tensor([0, 1], dtype=torch.int32, device=dev)
        rec = doc["kernel"] = {"runs": args.runs, "reps": args.reps, "sizes": {}}
        for n in args.sizes:
            k, k2 = scalars(n), scalars(2 * n, 4)                     # k2: [n, 2], the two exponents of an output side by side
            ka, kb = k2.reshape(n, 2, 32)[:, 0].contiguous(), k2.reshape(n, 2, 32)[:, 1].contiguous()
            x0, x1, out, dst = rep(two[0], n), rep(two[1], n), torch.empty(n, 384, dtype=torch.uint8, device=dev), torch.empty(n, 384, dtype=torch.uint8, device=dev)
            x01 = torch.stack([x0, x1], 1).contiguous()              # [n, 2, 384]: the factors of a segment side by side
            seg = torch.arange(0, 2 * n + 1, 2, dtype=torch.int64, device=dev)
            src = torch.empty_like(out)
            assert same(t1.pow(k), eng.gt_exp(x0, k))
            want = eng.gt_mul(eng.gt_exp(x0, ka), eng.gt_exp(x1, kb))
            assert same(t2.indexed(row, k2, terms=2)[0], want) and same(eng.gt_multi_exp(x01, k2, seg), want)
            legs = {"plain_copy_of_the_bytes_written": lambda: dst.copy_(src),
                    "indexed_terms_1": lambda: t1.pow(k, out=out), "gt_exp_on_the_replicated_base": lambda: eng.gt_exp(x0, k, out=out),
                    "indexed_terms_2": lambda: t2.indexed(row, k2, terms=2, out=out),
                    "two_gt_exp_then_gt_mul": lambda: eng.gt_mul(eng.gt_exp(x0, ka), eng.gt_exp(x1, kb)),
                    "gt_multi_exp_two_factor_segments": lambda: eng.gt_multi_exp(x01, k2, seg)}
            r = timed(legs)
            med = lambda leg: r[leg]["median_ms"]
            r.update({"elements": n, "bytes_written": n * 384,
                      "gt_exp_over_indexed_terms_1": med("gt_exp_on_the_replicated_base") / med("indexed_terms_1"),
                      "two_gt_exp_then_gt_mul_over_indexed_terms_2": med("two_gt_exp_then_gt_mul") / med("indexed_terms_2"),
                      "gt_multi_exp_over_indexed_terms_2": med("gt_multi_exp_two_factor_segments") / med("indexed_terms_2"),
                      "indexed_terms_1_over_plain_copy": med("indexed_terms_1") / med("plain_copy_of_the_bytes_written"),
                      "indexed_terms_1_M_per_s": n / med("indexed_terms_1") / 1e3})
            rec["sizes"][str(n)] = r
            print("kernel n = %d" % n, {name: round(v["median_ms"], 3) for name, v in r.items() if isinstance(v, dict)}, flush=True)
            save()
            del k, k2, ka, kb, x0, x1, x01, out, dst, src, want
        bases16 = eng.gt_exp(rep(e, 16), scalars(16, 5)).reshape(16, 384)
        rec["table_build"] = {"1_base": wall(lambda: eng.GTFixedBase(bases16[:1].contiguous()).close(), args.runs),
                              "16_bases": wall(lambda: eng.GTFixedBase(bases16).close(), args.runs), "table_bytes_per_base": t1.table_bytes()}
        print("table build", {name: round(v["median_ms"], 3) for name, v in rec["table_build"].items() if isinstance(v, dict)}, flush=True)
        save()
        return

    n = args.items
    if args.step == "waters05":
        alpha = scalars(1, 6)
        pts = eng.g2_scalar_mul_base(scalars(257, 7)).reshape(257, 128)
        table = waters05.hash_table(eng, pts[0].contiguous(), pts[1:].contiguous())
        e_alpha = eng.pair_batch(eng.g1_scalar_mul_base(alpha), put(g2)).reshape(384)
        gt_table = eng.GTFixedBase(e_alpha)
        masks = eng.random_bytes(SEED, (n + 1) // 2, stream=8, like=like).reshape(-1, 32)[:n].contiguous()         # 64-byte blocks: two digests each
        m, t = eng.gt_exp(rep(e, n), scalars(n, 9)).reshape(n, 384), scalars(n)
        plain = lambda: waters05.encrypt_batch(eng, table, e_alpha, m, masks, t)
        fixed = lambda: waters05.encrypt_batch(eng, table, e_alpha, m, masks, t, gt_table=gt_table)
        out = planner_legs("waters05_encrypt", n, {"gt_exp_route": plain, "with_gt_table": fixed}, lambda: all(same(a, b) for a, b in zip(plain(), fixed())))
        out["gt_exp_route_over_with_gt_table"] = out["calls"]["gt_exp_route"]["median_ms"] / out["calls"]["with_gt_table"]["median_ms"]
        save()
        return

    if args.step == "gentry06":
        g1_alpha = eng.g1_scalar_mul_base(scalars(1, 6)).reshape(64)
        h = eng.g2_scalar_mul_base(scalars(3, 7)).reshape(3, 128)
        e_gg, e_gh = gentry06.public_pairings(eng, put(g1), put(g2), h)
        m, ids, s = eng.gt_exp(rep(e, n), scalars(n, 9)).reshape(n, 384), scalars(n, 10), scalars(n)
        for name, k in (("gentry06_cpa_encrypt", 1), ("gentry06_cca_encrypt", 3)):
            gt_table = eng.GTFixedBase(torch.cat([e_gg.reshape(1, 384), e_gh[:k]]).contiguous())
            plain = lambda: gentry06.encrypt_batch(eng, g1_alpha, e_gg, e_gh[:k], m, ids, s)
            fixed = lambda: gentry06.encrypt_batch(eng, g1_alpha, e_gg, e_gh[:k], m, ids, s, gt_table=gt_table)
            out = planner_legs(name, n, {"gt_exp_route": plain, "with_gt_table": fixed}, lambda: all(same(a, b) for a, b in zip(plain(), fixed())))
            out["gt_exp_route_over_with_gt_table"] = out["calls"]["gt_exp_route"]["median_ms"] / out["calls"]["with_gt_table"]["median_ms"]
            save()
            gt_table.close()
        return

    if args.step == "bb04sibe":
        x, y = scalars(1, 6), scalars(1, 7)
        pp = bb04sibe.public_params(eng, x, y)
        gt_table = eng.GTFixedBase(e)
        ids, r, s, m = scalars(n, 10), scalars(n, 11), scalars(n), eng.gt_exp(rep(e, n), scalars(n, 9)).reshape(n, 384)
        keys = bb04sibe.keygen_batch(eng, x, y, ids, r)
        a, b, c = bb04sibe.encrypt_batch(eng, pp, gt_table, m, ids, s)
        a1, b1, c1 = bb04sibe.encrypt_batch(eng, pp, gt_table, m, ids[:1].expand(n, 32).contiguous(), s)             # every message to identity 0
        legs = {"keygen_batch": lambda: bb04sibe.keygen_batch(eng, x, y, ids, r), "encrypt_batch": lambda: bb04sibe.encrypt_batch(eng, pp, gt_table, m, ids, s),
                "decrypt_batch_a_key_per_ciphertext": lambda: bb04sibe.decrypt_batch(eng, a, b, c, r, keys),
                "decrypt_batch_one_key": lambda: bb04sibe.decrypt_batch(eng, a1, b1, c1, r[:1], keys[:1])}
        planner_legs("bb04sibe", n, legs, lambda: same(legs["decrypt_batch_a_key_per_ciphertext"](), m) and same(legs["decrypt_batch_one_key"](), m))
        return

    n, L = args.ibe_items, 256
    g1a, g2a, uij = bb04ibe.public_params(eng, scalars(1, 6), scalars(2 * L, 7))
    table, gt_table = bb04ibe.u_table(eng, uij), eng.GTFixedBase(bb04ibe.public_pairing(eng, g1a))
    names = eng.random_bytes(SEED, (n + 3) // 4, stream=8, like=like).reshape(-1)[:n * 16].contiguous()              # n identity strings of 16 bytes
    bits = bb04ibe.identity_bits_device(eng, names, torch.arange(0, n * 16 + 1, 16, dtype=torch.int64, device=dev)).contiguous()
    r, t, m = scalars(n * L, 11), scalars(n), eng.gt_exp(rep(e, n), scalars(n, 9)).reshape(n, 384)
    d0, dj = bb04ibe.keygen_batch(eng, table, g2a, bits, r)
    a, b, c = bb04ibe.encrypt_batch(eng, table, gt_table, m, bits, t)
    calls = {"keygen_batch": lambda en, tb, gt: bb04ibe.keygen_batch(en, tb, g2a, bits, r), "encrypt_batch": lambda en, tb, gt: bb04ibe.encrypt_batch(en, tb, gt, m, bits, t),
             "decrypt_batch_a_key_per_ciphertext": lambda en, tb, gt: bb04ibe.decrypt_batch(en, (d0, dj), a, b, c)}
    out = planner_legs("bb04ibe", n, {name: (lambda fn=fn: fn(eng, table, gt_table)) for name, fn in calls.items()},
                       lambda: same(bb04ibe.decrypt_batch(eng, (d0, dj), a, b, c), m))
    out.update({"identity_length": L, "u_table_bytes": table.table_bytes(), "split_ms": {}})
    for name, fn in calls.items():
        ms = {}
        fn(Split(eng, torch, ms), Split(table, torch, ms, "u_table."), Split(gt_table, torch, ms, "gt_table."))
        out["split_ms"][name] = {entry: sum(v) for entry, v in ms.items()}
        print("bb04ibe %s split:" % name, {entry: round(v, 2) for entry, v in out["split_ms"][name].items()}, flush=True)
    save()


if __name__ == "__main__":
    main()
