#!/usr/bin/env python3
"""The membership entries and the ASBB planner measured on one MI355X: ONE step per invocation, merged into profiles/membership.json
(run every step under a time limit of its own).

  --step g1 | g2 | gt
                  the entry at 2^20 HBM-resident elements, all of them group elements (no wavefront of the GT kernel skips its chain),
                  beside the only routes the entries before it offer and beside a plain device copy of the bytes the call reads — the
                  rate a kernel that computes nothing gets:
                      g1   g1_is_on_curve                       |  g1_marshal + g1_unmarshal
                      g2   g2_is_on_curve, g2_is_in_subgroup    |  g2_marshal + g2_unmarshal;  g2_scalar_mul by r
                      gt   gt_is_in_subgroup                    |  gt_exp(z, r) + gt_equal;  final_exp of as many values (the estimate of
                                                                   the issue: two of its three x^u chains)
                  The verdicts of the routes are compared first.  gt also times a batch of elements that are all outside the cyclotomic
                  subgroup: every wavefront skips.
  --step asbb     keygen / sign / verify_each / verify_batch (group 1024) / encrypt / decrypt at 2^16 items under one key, and
                  aggregate_public_keys over groups of 16 with and without validate.

Whole-call device times: after a warm-up, `runs` repetitions of `reps` calls between two device events, the legs of a comparison
alternating.  Planner calls: wall clock around a device synchronisation.  Not measured: host-pointer entries, more than one device.

    python tools/membership_bench.py --step gt [--runs 5] [--reps 3] [--out profiles/membership.json]
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

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
SEED = bytes(range(9, 41))


def stats(ms):
    return {"min_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "all_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=["g1", "g2", "gt", "asbb"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="calls back to back inside one timed window")
    ap.add_argument("--elements", type=int, default=1 << 20)
    ap.add_argument("--items", type=int, default=1 << 16)
    ap.add_argument("--planner-runs", type=int, default=3)
    ap.add_argument("--commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "membership.json"))
    args = ap.parse_args()
    import torch
    from gopairingbasedcryptography_amd import _build, agka09, bn254 as eng
    from gopairingbasedcryptography_amd.rng import Randomness
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
    doc.update({"what": "IsOnCurve / IsInSubGroup on in-memory G1, G2 and GT elements beside the routes of the entries before them and a plain copy; "
                        "the ASBB planner; one MI355X",
                "device": torch.cuda.get_device_name(0), "commit": commit, "date": time.strftime("%Y-%m-%d"),
                "timing": "kernels: warm-up, then `runs` repetitions of `reps` calls between two device events, legs alternating; planner calls: wall "
                          "clock around a device synchronisation",
                "not_measured": ["the host-pointer entries", "more than one device", "verify_batch over distinct keys"]})

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

    def wall(fn, runs):
        fn()
        ms = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return stats(ms)

    gen = torch.Generator(device=dev)
    gen.manual_seed(2009)
    scalars = lambda k: eng.fr_random(SEED, k, stream=3, like=torch.empty(0, dtype=torch.uint8, device=dev))
    r_rows = lambda k: torch.from_numpy(np.frombuffer(R.to_bytes(32, "little"), dtype=np.uint8).copy()).to(dev).reshape(1, 32).expand(k, 32).contiguous()

    def record(name, n, width, rec, ours):
        copy = rec["plain_copy_of_the_bytes_read"]["median_ms"]
        rec.update({"elements": n, "bytes_read": n * width, "runs": args.runs, "reps": args.reps})
        for leg in rec:
            if isinstance(rec[leg], dict) and leg != "plain_copy_of_the_bytes_read":
                rec[leg]["over_plain_copy"] = rec[leg]["median_ms"] / copy
                if leg not in ours:
                    rec[leg]["over_" + ours[0]] = rec[leg]["median_ms"] / rec[ours[0]]["median_ms"]
        doc[name] = rec
        print(name, {k: round(v["median_ms"], 3) for k, v in rec.items() if isinstance(v, dict)}, flush=True)
        save()

    if args.step in ("g1", "g2"):
        n, g2 = args.elements, args.step == "g2"
        width = 128 if g2 else 64
        pts = (eng.g2_scalar_mul_base if g2 else eng.g1_scalar_mul_base)(scalars(n)).reshape(n, width)
        ok = torch.empty(n, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(pts)
        marshal, unmarshal = (eng.g2_marshal, eng.g2_unmarshal) if g2 else (eng.g1_marshal, eng.g1_unmarshal)
        legs = {"plain_copy_of_the_bytes_read": lambda: dst.copy_(pts), "marshal_then_unmarshal": lambda: unmarshal(marshal(pts))}
        if g2:
            rr = r_rows(n)
            inf = torch.zeros(128, dtype=torch.uint8, device=dev)
            legs.update({"g2_is_on_curve": lambda: eng.g2_is_on_curve(pts, out=ok), "g2_is_in_subgroup": lambda: eng.g2_is_in_subgroup(pts, out=ok),
                         "g2_scalar_mul_by_r": lambda: eng.g2_scalar_mul(pts, rr)})
            assert bool((eng.g2_is_in_subgroup(pts) == 1).all()) and bool((eng.g2_is_on_curve(pts) == 1).all())
            assert bool((eng.g2_scalar_mul(pts, rr) == inf).all())
        else:
            legs["g1_is_on_curve"] = lambda: eng.g1_is_on_curve(pts, out=ok)
            assert bool((eng.g1_is_on_curve(pts) == 1).all())
        assert bool((unmarshal(marshal(pts))[1] == 1).all())
        record(args.step, n, width, timed(legs), ["g2_is_in_subgroup", "g2_is_on_curve"] if g2 else ["g1_is_on_curve"])
        return

    if args.step == "gt":
        n = args.elements
        g1, g2 = eng.generators()
        base = torch.from_numpy(np.ascontiguousarray(eng.pair_batch(g1, g2))).to(dev).reshape(1, 384)
        z = eng.gt_exp(base.expand(n, 384).contiguous(), scalars(n)).reshape(n, 384)
        noise = torch.randint(0, 256, (n, 384), dtype=torch.uint8, device=dev, generator=gen)      # random Fp12 elements: none is cyclotomic
        noise.reshape(n, 12, 32)[:, :, 31] &= 0x1f                                                 # top byte below 0x20: every coordinate below p
        ok = torch.empty(n, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(z)
        rr = r_rows(n)
        one = torch.from_numpy(np.ascontiguousarray(eng.gt_exp(base.cpu().numpy(), [0]))).to(dev).reshape(-1)
        assert bool((eng.gt_is_in_subgroup(z) == 1).all()) and bool((eng.gt_equal(eng.gt_exp(z, rr), one) == 1).all())
        assert not bool(eng.gt_is_in_subgroup(noise).any())
        legs = {"plain_copy_of_the_bytes_read": lambda: dst.copy_(z), "gt_is_in_subgroup": lambda: eng.gt_is_in_subgroup(z, out=ok),
                "gt_is_in_subgroup_every_wavefront_skips": lambda: eng.gt_is_in_subgroup(noise, out=ok),
                "gt_exp_by_r_then_gt_equal": lambda: eng.gt_equal(eng.gt_exp(z, rr, out=dst), one, out=ok), "final_exp_of_as_many": lambda: eng.final_exp(z)}
        record("gt", n, 384, timed(legs), ["gt_is_in_subgroup", "gt_is_in_subgroup_every_wavefront_skips"])
        return

    n = args.items
    like = torch.empty(0, dtype=torch.uint8, device=dev)
    out = doc["asbb"] = {"items": n, "planner_runs": args.planner_runs, "calls": {}}
    rr, xx = eng.fr_random(SEED, 1, stream=1, like=like), eng.fr_random(SEED, 1, stream=2, like=like)
    R1, A1, X1 = (v[0] for v in agka09.keygen_batch(eng, rr, xx))
    msgs = torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device=dev, generator=gen)
    H = agka09.hash_strings(eng, msgs, torch.arange(0, n * 32 + 1, 32, dtype=torch.int64, device=dev))
    sig = agka09.sign_batch(eng, rr, X1, hashed=H)
    m = eng.gt_exp(A1.reshape(1, 384).expand(n, 384).contiguous(), scalars(n)).reshape(n, 384)
    c1, c2, c3 = agka09.encrypt_batch_seeded(eng, R1, A1, m, Randomness(eng, SEED))
    assert bool((agka09.verify_each(eng, R1, A1, sig, hashed=H) == 1).all())
    assert bool((agka09.verify_batch(eng, R1, A1, sig, Randomness(eng, SEED), hashed=H, group=1024) == 1).all())
    assert bool((agka09.decrypt_batch(eng, c1, c2, c3, sig, hashed=H) == m).all())
    kr, kx = scalars(n), eng.fr_random(SEED, n, stream=4, like=like)
    Rn, An, _ = agka09.keygen_batch(eng, kr, kx)
    seg = np.arange(0, n + 1, 16)
    calls = {"keygen_batch": lambda: agka09.keygen_batch(eng, kr, kx), "sign_batch": lambda: agka09.sign_batch(eng, rr, X1, hashed=H),
             "verify_each": lambda: agka09.verify_each(eng, R1, A1, sig, hashed=H),
             "verify_batch_group_1024": lambda: agka09.verify_batch(eng, R1, A1, sig, Randomness(eng, SEED), hashed=H, group=1024),
             "encrypt_batch_seeded": lambda: agka09.encrypt_batch_seeded(eng, R1, A1, m, Randomness(eng, SEED)),
             "decrypt_batch": lambda: agka09.decrypt_batch(eng, c1, c2, c3, sig, hashed=H),
             "aggregate_public_keys_groups_of_16": lambda: agka09.aggregate_public_keys(eng, Rn, An, seg),
             "aggregate_public_keys_groups_of_16_validate": lambda: agka09.aggregate_public_keys(eng, Rn, An, seg, validate=True)}
    for name, fn in calls.items():
        out["calls"][name] = wall(fn, args.planner_runs)
        print("asbb %s: %.2f ms" % (name, out["calls"][name]["median_ms"]), flush=True)
        save()
    out["verify_each_over_verify_batch"] = out["calls"]["verify_each"]["median_ms"] / out["calls"]["verify_batch_group_1024"]["median_ms"]
    out["validate_over_plain_aggregation"] = (out["calls"]["aggregate_public_keys_groups_of_16_validate"]["median_ms"] /
                                              out["calls"]["aggregate_public_keys_groups_of_16"]["median_ms"])
    save()


if __name__ == "__main__":
    main()
