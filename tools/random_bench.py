#!/usr/bin/env python3
"""The seed-addressed generator measured on one MI355X, in one process: writes profiles/device_random.json.

  (1) fr_random and random_bytes at 2^24 elements into HBM-resident buffers: after one warm-up, RUNS repetitions, each REPS calls
      back to back between two device events; min, median and max, and the bytes written per second beside the HBM peak (the kernels read nothing);
  (2) the route fr_random replaces, for the same 2^24 scalars: os.urandom -> 64-byte strings -> reduction modulo r in Python integers or
      through a numpy object array (both timed on --host-sample strings, the faster one named and run over all of them) -> a pinned
      host buffer -> one copy to the device, every stage by the wall clock;
  (3) bsw07.encrypt_batch_seeded against bsw07.encrypt_batch on device-resident randomness at 2^12 and 2^16 ciphertexts x 256 leaves
      (256-of-256), whole calls by the wall clock with a device synchronisation, the two alternating;
  (4) optionally the headline lines of bench.py runs on the parent commit's library and on this tree's (--bench-parent / --bench-this:
      files holding one JSON line per run, in the order they were run), copied in side by side.

    python tools/random_bench.py [--runs 5] [--commit ID] [--out profiles/device_random.json]
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

HBM_PEAK_BYTES_PER_S = 8.0e12          # MI355X: 8 TB/s
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def stats(ms):
    return {"min_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "all_ms": ms}


def reduce_python(raw):
    """64-byte strings -> 32-byte little-endian scalars, one Python integer at a time"""
    view, from_bytes = memoryview(raw), int.from_bytes
    return b"".join([(from_bytes(view[i:i + 64], "big") % R).to_bytes(32, "little") for i in range(0, len(raw), 64)])


def reduce_numpy(raw):
    """the same through a numpy object array: the eight 64-bit words of a string combined and reduced elementwise"""
    words = np.frombuffer(raw, dtype=">u8").reshape(-1, 8).astype(object)
    acc = words[:, 0]
    for j in range(1, 8):
        acc = (acc << 64) | words[:, j]
    acc = acc % R
    out = np.empty((len(acc), 4), dtype="<u8")
    mask = (1 << 64) - 1
    for j in range(4):
        out[:, j] = ((acc >> (64 * j)) & mask).astype(np.uint64)
    return out.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="calls back to back inside one timed window of a device entry")
    ap.add_argument("--elements", type=int, default=1 << 24)
    ap.add_argument("--host-sample", type=int, default=1 << 18, help="strings on which the two host reductions are compared")
    ap.add_argument("--ciphertexts", type=int, nargs="*", default=[1 << 12, 1 << 16], help="none: skip the planner")
    ap.add_argument("--leaves", type=int, default=256)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--commit")
    ap.add_argument("--bench-parent")
    ap.add_argument("--bench-this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_random.json"))
    args = ap.parse_args()
    import torch
    from gopairingbasedcryptography_amd import _build, bn254 as eng, bsw07, rng as rng_mod
    _build.build_library()
    eng.init(0)
    dev = torch.device("cuda", 0)
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
    n = args.elements
    seed = bytes(range(32))
    doc = {"what": "fr_random, random_bytes and bsw07.encrypt_batch_seeded beside the host-made randomness they replace, one MI355X",
           "device": torch.cuda.get_device_name(0), "commit": commit, "date": time.strftime("%Y-%m-%d"), "runs": args.runs, "reps": args.reps,
           "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
           "timing": "every shape warmed up once; device entries: `runs` repetitions, each `reps` calls back to back between two device events, over reps (one call alone is a window that measures the clock); host stages and "
                     "whole planner calls: wall clock, with a device synchronisation where the device takes part; min, median and max"}

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

    # ---- (1) the two entries alone
    entries = {}
    for name, width in (("fr_random", 32), ("random_bytes", 64)):
        out = torch.empty(n * width, dtype=torch.uint8, device=dev)
        fn = getattr(eng, name)
        rec = timed(lambda: fn(seed, n, stream=1, out=out))
        rate = n * width / (rec["median_ms"] * 1e-3)
        rec.update({"elements": n, "bytes_written": n * width, "bytes_per_s": rate, "fraction_of_hbm_peak": rate / HBM_PEAK_BYTES_PER_S,
                    "elements_per_s": n / (rec["median_ms"] * 1e-3)})
        entries[name] = rec
        print("%s x %d: %.3f ms median (%.3f - %.3f), %.2f TB/s written = %.1f %% of the HBM peak" % (
            name, n, rec["median_ms"], rec["min_ms"], rec["max_ms"], rate / 1e12, 100 * rate / HBM_PEAK_BYTES_PER_S), flush=True)
        del out
    # a plain device fill of the same bytes: the store rate this chip gives a kernel that computes nothing
    for name, width in (("fill_32_bytes_per_element", 32), ("fill_64_bytes_per_element", 64)):
        out = torch.empty(n * width, dtype=torch.uint8, device=dev)
        rec = timed(lambda: out.fill_(7))
        rec.update({"bytes_written": n * width, "bytes_per_s": n * width / (rec["median_ms"] * 1e-3)})
        entries[name] = rec
        del out
    for name, fill in (("fr_random", "fill_32_bytes_per_element"), ("random_bytes", "fill_64_bytes_per_element")):
        entries[name]["fraction_of_plain_fill_rate"] = entries[name]["bytes_per_s"] / entries[fill]["bytes_per_s"]
    doc["device_entries"] = entries
    save()

    # ---- (2) the host route for the same scalars
    if not args.skip_host:
        def wall(fn, runs):
            ms, res = [], None
            for _ in range(runs):
                t0 = time.perf_counter()
                res = fn()
                ms.append((time.perf_counter() - t0) * 1e3)
            return stats(ms), res
        host = {"elements": n}
        host["os_urandom"], raw = wall(lambda: os.urandom(64 * n), 1)
        m = min(args.host_sample, n)
        sample = raw[:64 * m]
        pick = {}
        for name, fn in (("python_integers", reduce_python), ("numpy_object_array", reduce_numpy)):
            pick[name], got = wall(lambda: fn(sample), 2)
            pick[name]["strings"] = m
            pick[name]["us_per_scalar"] = pick[name]["min_ms"] * 1e3 / m
            assert got == reduce_python(sample)
        fastest = min(pick, key=lambda k: pick[k]["min_ms"])
        host["reductions_on_a_sample"], host["fastest_reduction"] = pick, fastest
        host["reduction"], scalars = wall(lambda: (reduce_python if fastest == "python_integers" else reduce_numpy)(raw), 1)
        arr = np.frombuffer(scalars, dtype=np.uint8)
        pinned = torch.empty(arr.size, dtype=torch.uint8).pin_memory()
        target = torch.empty(arr.size, dtype=torch.uint8, device=dev)

        def upload():
            pinned.numpy()[:] = arr
            target.copy_(pinned, non_blocking=True)
            torch.cuda.synchronize()
        upload()
        host["pinned_copy_and_upload"], _ = wall(upload, args.runs)
        total = host["os_urandom"]["median_ms"] + host["reduction"]["median_ms"] + host["pinned_copy_and_upload"]["median_ms"]
        host["total_ms"] = total
        host["over_fr_random"] = total / entries["fr_random"]["median_ms"]
        host["note"] = "os.urandom and the full reduction are timed once (they take seconds); the two reductions are compared on a sample, best of two"
        doc["host_route"] = host
        print("host route x %d: urandom %.0f ms + %s %.0f ms + pinned copy %.1f ms = %.0f ms, %.0f x fr_random" % (
            n, host["os_urandom"]["median_ms"], fastest, host["reduction"]["median_ms"], host["pinned_copy_and_upload"]["median_ms"], total, host["over_fr_random"]), flush=True)
        del raw, scalars, arr, pinned, target
        save()

    # ---- (3) BSW07 Encrypt: seeded against device-resident randomness handed in
    if args.ciphertexts:
        L = args.leaves
        nprng = np.random.default_rng(2007)
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        rand = lambda *shape: put(nprng.integers(0, 256, size=shape + (32,), dtype=np.uint8))
        g1, g2 = (put(x) for x in eng.generators())
        e = eng.pair_batch(g1, g2)
        e_alpha = eng.gt_exp(e.reshape(-1), rand(1).reshape(-1)).reshape(-1)
        hpk = eng.g1_scalar_mul(g1, rand(1).reshape(-1)).reshape(-1)
        H1 = eng.g1_scalar_mul_base(rand(L).reshape(-1)).reshape(L, 64).cpu().numpy()
        h1 = {a: H1[a] for a in range(L)}
        plan = bsw07.share_plan(bsw07.Threshold(L, *[bsw07.Leaf(a) for a in range(L)]))
        C = L - 1
        doc["bsw07_encrypt"] = []
        for k in args.ciphertexts:
            messages = eng.gt_exp(e.expand(k, 384).contiguous().reshape(-1), rand(k).reshape(-1)).reshape(k, 384)
            s, coeffs = rand(k), rand(k, C)
            draws = rng_mod.Randomness(eng, seed)
            legs = {"encrypt_batch_seeded": lambda: bsw07.encrypt_batch_seeded(eng, plan, hpk, e_alpha, h1, messages, draws),
                    "encrypt_batch": lambda: bsw07.encrypt_batch(eng, plan, hpk, e_alpha, h1, messages, s, coeffs),
                    "the_two_draws_alone": lambda: (eng.fr_random(seed, k, stream=0, like=messages), eng.fr_random(seed, k * C, stream=1, like=messages))}
            for fn in legs.values():
                fn()
            torch.cuda.synchronize()
            ms = {name: [] for name in legs}
            for _ in range(args.runs):
                for name, fn in legs.items():
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    ms[name].append((time.perf_counter() - t0) * 1e3)
            rec = {"ciphertexts": k, "leaves": L, "policy": "%d-of-%d" % (L, L), "scalars_drawn": k * (1 + C), "bytes_of_randomness": k * (1 + C) * 32}
            rec.update({name: stats(v) for name, v in ms.items()})
            rec["seeded_over_handed_in"] = rec["encrypt_batch_seeded"]["median_ms"] / rec["encrypt_batch"]["median_ms"]
            doc["bsw07_encrypt"].append(rec)
            print("bsw07 x %d x %d: seeded %.1f ms, randomness handed in %.1f ms, the draws alone %.3f ms" % (
                k, L, rec["encrypt_batch_seeded"]["median_ms"], rec["encrypt_batch"]["median_ms"], rec["the_two_draws_alone"]["median_ms"]), flush=True)
            del messages, s, coeffs
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
