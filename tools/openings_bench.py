#!/usr/bin/env python3
"""Fused opening proofs and the GWWW25 planners measured on one MI355X: ONE step per invocation, merged into profiles/openings.json (run
every step under a time limit of its own).

  --step kernel   FixedBase.openings beside the route it replaces, fr_poly_quotients + FixedBase.msm chunk by chunk through one 256 MB
                  scratch buffer with a flag read back per chunk (what afp25.opening_proofs does), in the same run, G1 and G2, under a table
                  of 257 bases: 2^16 identities in full batches of 256, then the same identities in batches of 32.  The batch polynomials
                  are made beforehand by each route's own kernel (and timed on their own); the outputs are compared first.  Peak extra
                  device memory of both routes as the torch allocator sees it (workspaces, scratch and outputs; the library's own block
                  table is a few kilobytes).
  --step gwww25   gwww25 keygen, encrypt (both forms), digests, compute_key and decrypt at 2^16 items in 256 batches of B = 256, with
                  the time per engine entry inside decrypt (every entry between two device synchronisations: the split adds up to more
                  than the whole call's time)

Device times: after a warm-up, `runs` repetitions of one call between two device events, the legs of a comparison alternating (the old
route synchronises inside, so its window holds its waits, as a caller sees them).  Planner calls: wall clock around a device
synchronisation.  Not measured: host-pointer entries, more than one device.

    python tools/openings_bench.py --step kernel [--runs 5] [--out profiles/openings.json]
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

SEED = bytes(range(17, 49))
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
TAU = 0x1F3A5C7E9B2D4F60718293A4B5C6D7E8F9010A1B2C3D4E5F60718293A4B5C6D % R
SCRATCH_BYTES = 256 << 20


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
    ap.add_argument("--step", required=True, choices=["kernel", "gwww25"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--items", type=int, default=1 << 16)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--short", type=int, default=32)
    ap.add_argument("--planner-runs", type=int, default=3)
    ap.add_argument("--commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "openings.json"))
    args = ap.parse_args()
    import torch
    from gopairingbasedcryptography_amd import _build, bn254 as eng, gwww25
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
    doc.update({"what": "FixedBase.openings (quotient coefficients made in the lane that adds their terms) beside fr_poly_quotients + FixedBase.msm through a "
                        "256 MB scratch buffer; the GWWW25 planners; one MI355X, one run",
                "device": torch.cuda.get_device_name(0), "commit": commit, "date": time.strftime("%Y-%m-%d"),
                "timing": "kernels: warm-up, then `runs` repetitions of one call between two device events, legs alternating; planner calls: wall clock "
                          "around a device synchronisation",
                "not_measured": ["the host-pointer entries", "more than one device", "batches longer than 256 (the 1024-coefficient staging)"]})

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
                fn()
                b.record()
                b.synchronize()
                ms[name].append(a.elapsed_time(b))
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

    def peak_extra(fn):
        """bytes the torch allocator's peak rises by during one call (the result is dropped before the next measurement)"""
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    like = torch.empty(0, dtype=torch.uint8, device=dev)
    scalars = lambda k, stream=3: eng.fr_random(SEED, k, stream=stream, like=like)
    n = args.items

    if args.step == "kernel":
        ids = scalars(n).reshape(-1)
        res = doc.setdefault("kernel", {})
        for g2 in (False, True):
            group = "g2" if g2 else "g1"
            nbase = args.batch + 1
            powers = (eng.g2_scalar_mul_base if g2 else eng.g1_scalar_mul_base)([pow(TAU, c, R) for c in range(nbase)])
            table = eng.FixedBase(np.asarray(powers), g2=g2)
            width = table.width

            def old_route(B, coeffs):
                """afp25.opening_proofs with B free: quotient rows chunk by chunk of whole batches through ONE scratch buffer, a flag read
                back per chunk"""
                k, per_batch = n // B, B * nbase * 32
                chunk = min(k, max(1, SCRATCH_BYTES // per_batch))
                scratch = torch.empty(chunk * per_batch, dtype=torch.uint8, device=dev)
                okbuf = torch.empty(chunk * B, dtype=torch.uint8, device=dev)
                pi = torch.empty((n, width), dtype=torch.uint8, device=dev)
                c = coeffs.reshape(-1)
                for lo in range(0, k, chunk):
                    m = min(chunk, k - lo)
                    q, ok = eng.fr_poly_quotients(c[lo * (B + 1) * 32:(lo + m) * (B + 1) * 32], ids[lo * B * 32:(lo + m) * B * 32], B, nbase, out=scratch[:m * per_batch], ok=okbuf[:m * B])
                    pi[lo * B:(lo + m) * B] = table.msm(q)
                    if not bool(ok.all()):
                        raise ValueError("identity not found in identity list")
                return pi

            for B in (args.batch, args.short):
                old_coeffs = eng.fr_poly_from_roots(ids, B)
                new_coeffs = eng.fr_poly_from_roots_segments(ids, B, nbase)
                fused = lambda: table.openings(ids, B, coeffs=new_coeffs.reshape(-1))
                pts, ok = fused()
                same = bool(ok.all()) and torch.equal(pts, old_route(B, old_coeffs)) and torch.equal(new_coeffs[:, :B + 1].contiguous(), old_coeffs)
                if not same:
                    raise SystemExit("%s, batches of %d: the two routes disagree" % (group, B))
                entry = {"identities": n, "batch": B, "nbase": nbase, "outputs_equal": same}
                entry.update(timed({"fused_openings": fused, "quotients_plus_msm": lambda: old_route(B, old_coeffs)}))
                entry.update(timed({"from_roots_segments": lambda: eng.fr_poly_from_roots_segments(ids, B, nbase), "from_roots": lambda: eng.fr_poly_from_roots(ids, B)}))
                entry["peak_extra_bytes"] = {"fused_openings": peak_extra(fused), "quotients_plus_msm": peak_extra(lambda: old_route(B, old_coeffs))}
                entry["workspace_bytes"] = int(eng._lib.load().gpbc_fixed_base_openings_workspace_bytes(table._h, n))
                res["%s_batches_of_%d" % (group, B)] = entry
                print(group, B, {k: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else v) for k, v in entry.items()}, flush=True)
                save()
            table.close()

    if args.step == "gwww25":
        B, k = args.batch, n // args.batch
        counts = [B] * k
        tau, w, v, h, alpha = (int.from_bytes(bytes(r), "little") for r in scalars(5, stream=9).cpu().numpy().reshape(5, 32))
        res = doc.setdefault("gwww25", {"items": n, "B": B, "batches": k})
        res["keygen"] = wall(lambda: gwww25.keygen(eng, B, tau, w, v, h, alpha))
        mpk = gwww25.keygen(eng, B, tau, w, v, h, alpha)
        t0 = time.perf_counter()
        table = gwww25.srs_table(eng, mpk)
        tables = gwww25.encrypt_tables(eng, mpk)
        torch.cuda.synchronize()
        res["tables_build_ms"] = (time.perf_counter() - t0) * 1e3
        e = torch.from_numpy(np.asarray(eng.pair_batch(*eng.generators()))).to(dev).reshape(1, 384)
        messages = eng.gt_exp(e.expand(n, 384).contiguous().reshape(-1), scalars(n, stream=4).reshape(-1)).reshape(n, 384)
        ids, s = scalars(n, stream=5).reshape(-1), scalars(n, stream=6).reshape(-1)
        tg, r, y = scalars(k, stream=7).reshape(-1), scalars(k, stream=8).reshape(-1), scalars(k, stream=10).reshape(-1)
        tg_items = tg.reshape(k, 1, 32).expand(k, B, 32).contiguous().reshape(-1)
        plain = gwww25.encrypt_batch(eng, mpk, messages, ids, tg_items, s)
        fast = gwww25.encrypt_batch(eng, mpk, messages, ids, tg_items, s, tables=tables)
        if not all(torch.equal(a, b) for a, b in zip(plain, fast)):
            raise SystemExit("encrypt: the tables path disagrees")
        res["encrypt"] = wall(lambda: gwww25.encrypt_batch(eng, mpk, messages, ids, tg_items, s))
        res["encrypt_tables"] = wall(lambda: gwww25.encrypt_batch(eng, mpk, messages, ids, tg_items, s, tables=tables))
        res["digests"] = wall(lambda: gwww25.digests(eng, table, ids, counts))
        D = gwww25.digests(eng, table, ids, counts)
        msk = (w, v, h, alpha)
        res["compute_key"] = wall(lambda: gwww25.compute_key_batch(eng, msk, D, tg, r, y))
        sk = gwww25.compute_key_batch(eng, msk, D, tg, r, y)
        m, ok = gwww25.decrypt_batches(eng, table, ids, counts, sk, plain)
        if not (bool(ok.all()) and torch.equal(m, messages)):
            raise SystemExit("decrypt(encrypt(M)) != M")
        res["round_trip_ok"] = True
        res["decrypt"] = wall(lambda: gwww25.decrypt_batches(eng, table, ids, counts, sk, plain))
        split = {}
        gwww25.decrypt_batches(Split(eng, torch, split), Split(table, torch, split, "table."), ids, counts, sk, plain)
        res["decrypt_split_ms"] = {name: sum(v) for name, v in split.items()}
        print({key: (val["median_ms"] if isinstance(val, dict) and "median_ms" in val else val) for key, val in res.items()}, flush=True)
        save()
        for t in (table,) + tuple(tables):
            t.close()


if __name__ == "__main__":
    main()
