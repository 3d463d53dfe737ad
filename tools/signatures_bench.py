#!/usr/bin/env python3
"""Segmented inner products in Fr and the signature planners measured on one MI355X: ONE step per invocation, merged into
profiles/signatures.json (run every step under a time limit of its own).

  --step fr_dot   gpbc_fr_dot_segments_dev at 2^20 HBM-resident elements in 1, 2^10 and 2^16 segments, with a second operand (dot) and
                  without (sum): the C entry alone (caller's workspace and output, table in device memory), the Python wrapper
                  bn254.fr_dot_segments on the same buffers, and a plain device copy of the bytes the call reads (64 / 32 bytes per
                  element) — the rate a kernel that computes nothing gets; the ratio to it is what the kernel is judged by.  Once per
                  shape: the only prior route, the array read to the host and summed in Python integers, whose result is compared.
  --step zss04 | bb04 | bls01
                  verify_batch against verify_each at 2^16 signatures under one key, group in {64, 1024, 2^16}, all valid and with 1 %
                  forged (655 signatures replaced by their neighbour's); the verdicts of the two are compared first.  verify_each uses
                  only entries older than this file's subject and is the baseline.  The weights are drawn inside the timed call.
                  One more verify_batch call per case goes through an engine whose every call is timed between two device
                  synchronisations: the stages of the call.

Kernels: after a warm-up, `runs` repetitions of `reps` calls between two device events, the legs of a comparison alternating.
Planner calls: wall clock around a device synchronisation, `planner_runs` repetitions, alternating.  Not measured: host-pointer
entries, more than one device.

    python tools/signatures_bench.py --step fr_dot [--runs 7] [--reps 20] [--out profiles/signatures.json]
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
SEED = bytes(range(7, 39))


def stats(ms):
    return {"min_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "all_ms": ms}


class Staged:
    """an engine whose every call is timed between two device synchronisations and added up under its name"""

    def __init__(self, engine, torch):
        self._engine, self._torch, self.ms = engine, torch, {}

    def __getattr__(self, name):
        fn = getattr(self._engine, name)
        if not callable(fn):
            return fn

        def timed(*a, **kw):
            self._torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn(*a, **kw)
            self._torch.cuda.synchronize()
            self.ms[name] = self.ms.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
            return res
        return timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", required=True, choices=["fr_dot", "zss04", "bb04", "bls01"])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="calls back to back inside one timed window")
    ap.add_argument("--elements", type=int, default=1 << 20)
    ap.add_argument("--signatures", type=int, default=1 << 16)
    ap.add_argument("--planner-runs", type=int, default=5)
    ap.add_argument("--commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "signatures.json"))
    args = ap.parse_args()
    import torch
    from gopairingbasedcryptography_amd import _build, _lib, bb04sig, bls01, zss04, bn254 as eng
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
    doc.update({"what": "fr_dot_segments beside a plain copy and the host route; verify_batch beside verify_each for ZSS04, BB04 and BLS01; one MI355X",
                "device": torch.cuda.get_device_name(0), "commit": commit, "date": time.strftime("%Y-%m-%d"),
                "timing": "kernels: warm-up, then `runs` repetitions of `reps` calls between two device events, legs alternating; planner calls: wall "
                          "clock around a device synchronisation, legs alternating",
                "not_measured": ["the host-pointer entries", "more than one device", "a key per signature", "128-bit weights"]})

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

    def wall(legs, runs):
        for fn in legs.values():
            fn()
        ms = {name: [] for name in legs}
        for _ in range(runs):
            for name, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3)
        return {name: stats(v) for name, v in ms.items()}

    gen = torch.Generator(device=dev)
    gen.manual_seed(2004)

    if args.step == "fr_dot":
        n = args.elements
        lib = _lib.load()
        a = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        b = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        dst = torch.empty((2 * n, 32), dtype=torch.uint8, device=dev)
        src = torch.cat([a, b])
        st = torch.cuda.current_stream().cuda_stream
        out = doc["fr_dot_segments"] = {"elements": n, "runs": args.runs, "reps": args.reps, "shapes": {}}
        for n_seg in (1, 1 << 10, 1 << 16):
            seg = np.arange(0, n + 1, n // n_seg, dtype=np.int64)
            dseg = torch.from_numpy(seg).to(dev)
            res = torch.empty((n_seg, 32), dtype=torch.uint8, device=dev)
            wsb = lib.gpbc_fr_dot_segments_workspace_bytes(n, n_seg)
            ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
            for mode, bb, nb, moved in (("dot", b, n, 64 * n), ("sum", None, 0, 32 * n)):
                entry = lambda: _lib.check(lib.gpbc_fr_dot_segments_dev(a.data_ptr(), bb.data_ptr() if bb is not None else None, nb, dseg.data_ptr(), n, n_seg,
                                                                        res.data_ptr(), ws.data_ptr(), wsb, st))
                legs = {"c_entry": entry,
                        "python_wrapper": lambda: eng.fr_dot_segments(a, bb, dseg, out=res, workspace=ws),
                        "plain_copy_of_the_bytes_read": lambda: dst.reshape(-1)[:moved].copy_(src.reshape(-1)[:moved])}
                rec = timed(legs)
                got = res.cpu().numpy().copy()
                t0 = time.perf_counter()
                ha, hb = a.cpu().numpy(), None if bb is None else bb.cpu().numpy()
                ia = [int.from_bytes(r.tobytes(), "little") for r in ha]
                ib = None if hb is None else [int.from_bytes(r.tobytes(), "little") for r in hb]
                sums = [sum(ia[i] * (ib[i] if ib is not None else 1) for i in range(int(lo), int(hi))) % R for lo, hi in zip(seg[:-1], seg[1:])]
                host_ms = (time.perf_counter() - t0) * 1e3
                same = [int.from_bytes(r.tobytes(), "little") for r in got] == sums
                assert same, (n_seg, mode)
                rec.update({"bytes_read": moved, "workspace_bytes": wsb, "host_route_read_back_and_python_integers_ms": host_ms, "equal_to_python_integers": same,
                            "c_entry_over_plain_copy": rec["c_entry"]["median_ms"] / rec["plain_copy_of_the_bytes_read"]["median_ms"],
                            "bytes_per_s": moved / (rec["c_entry"]["median_ms"] * 1e-3),
                            "host_route_over_c_entry": host_ms / rec["c_entry"]["median_ms"]})
                out["shapes"]["%d_segments_%s" % (n_seg, mode)] = rec
                print("fr_dot %s, %d segments: entry %.4f ms, wrapper %.4f ms, copy %.4f ms (x%.2f), host route %.0f ms" % (
                    mode, n_seg, rec["c_entry"]["median_ms"], rec["python_wrapper"]["median_ms"], rec["plain_copy_of_the_bytes_read"]["median_ms"],
                    rec["c_entry_over_plain_copy"], host_ms), flush=True)
                save()
        return

    n = args.signatures
    scal = lambda: torch.from_numpy(np.frombuffer(b"".join((int.from_bytes(os.urandom(40), "big") % R).to_bytes(32, "little") for _ in range(n)),
                                                  dtype=np.uint8).copy()).to(dev).reshape(n, 32)
    rs = np.random.default_rng(2004)
    forged_at = np.sort(rs.choice(n, size=max(1, n // 100), replace=False))
    x, x2 = 0x1234567 + (1 << 200), 0x7654321 + (1 << 199)

    def forge(sig):
        f = sig.clone()
        idx = torch.from_numpy(forged_at).to(dev)
        f[idx] = sig[(idx + 1) % n]
        return f

    if args.step == "zss04":
        eg, P = zss04.public_params(eng), zss04.keygen_batch(eng, [x])[0]
        hm = scal()
        S = zss04.sign_batch(eng, x, hm=hm)
        each = lambda s: zss04.verify_each(eng, P, eg, s, hm=hm)
        batch = lambda s, g, e=eng: zss04.verify_batch(e, P, eg, s, Randomness(e, SEED), hm=hm, group=g)
    elif args.step == "bb04":
        eg = bb04sig.public_params(eng)
        Y, Z = (k[0] for k in bb04sig.keygen_batch(eng, [x], [x2]))
        m = scal()
        r, S = bb04sig.sign_batch_seeded(eng, x, x2, m, Randomness(eng, bytes(32)))
        each = lambda s: bb04sig.verify_each(eng, Y, Z, eg, m.reshape(-1), r, s)
        batch = lambda s, g, e=eng: bb04sig.verify_batch(e, Y, Z, eg, m.reshape(-1), r, s, Randomness(e, SEED), group=g)
    else:
        g1, X = bls01.public_params(eng), bls01.keygen_batch(eng, [x])[0]
        msgs = torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device=dev, generator=gen)
        H = bls01.hash_messages(eng, msgs, torch.arange(0, n * 32 + 1, 32, dtype=torch.int64, device=dev))
        S = bls01.sign_batch(eng, torch.from_numpy(np.frombuffer(x.to_bytes(32, "little"), dtype=np.uint8).copy()).to(dev), hashed=H)
        each = lambda s: bls01.verify_each(eng, X, g1, s, hashed=H)
        batch = lambda s, g, e=eng: bls01.verify_batch(e, X, g1, s, Randomness(e, SEED), hashed=H, group=g)
    out = doc[args.step] = {"signatures": n, "forged": int(forged_at.size), "planner_runs": args.planner_runs, "cases": {}}
    for label, sig in (("all_valid", S), ("one_percent_forged", forge(S))):
        want = each(sig)
        assert int(want.sum()) == (n if label == "all_valid" else n - forged_at.size), label
        for group in (64, 1024, n):
            assert bool((batch(sig, group) == want).all()), (label, group)
            failing_groups = len({int(p) // group for p in forged_at}) if label != "all_valid" else 0
            rec = wall({"verify_each": lambda: each(sig), "verify_batch": lambda: batch(sig, group)}, args.planner_runs)
            rec.update({"group": group, "groups": -(-n // group), "failing_groups": failing_groups,
                        "verify_each_over_verify_batch": rec["verify_each"]["median_ms"] / rec["verify_batch"]["median_ms"]})
            staged = Staged(eng, torch)                                     # one more call, every engine call between two synchronisations
            t0 = time.perf_counter()
            batch(sig, group, staged)
            rec["verify_batch_by_engine_call_ms"] = dict(staged.ms, whole_call=(time.perf_counter() - t0) * 1e3)
            out["cases"]["%s_group_%d" % (label, group)] = rec
            print("%s %s, group %d (%d of %d groups fail): verify_each %.2f ms, verify_batch %.2f ms (x%.2f)" % (
                args.step, label, group, failing_groups, rec["groups"], rec["verify_each"]["median_ms"], rec["verify_batch"]["median_ms"],
                rec["verify_each_over_verify_batch"]), flush=True)
            save()


if __name__ == "__main__":
    main()
