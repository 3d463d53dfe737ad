#!/usr/bin/env python3
"""The XOR mask from GT bytes and the Boneh-Franklin planner measured on one MI355X, in one process: writes profiles/gt_xor_mask.json.

  (1) gt_xor_mask on HBM-resident tensors at 2^20 items, rows of 32 and of 384 bytes, into a given output and in place;
  (2) the route it replaces on the same inputs: gt_marshal (all 384 bytes of every element) + torch.bitwise_xor on the first `width`
      columns — the two routes alternate inside every repetition, and their outputs are compared byte for byte before anything is timed;
  (3) a ragged batch whose lengths cycle through 1 ... 64 (flat buffer plus offsets) beside the same bytes as padded rows of 64, rows of
      33 bytes (every piece at an odd address: the byte path), and the offset form on messages of 384 bytes beside the same rows in
      the row form (the two lane orders on the same work);
  (4) a plain device copy of the bytes each call moves at the least — 32 ceil(L / 32) of the 384 bytes of every GT element, the message
      read and the output written — which is the rate a kernel that computes nothing gets;
  (5) bf01.keygen_batch, encrypt_batch and decrypt_batch (one key) at 2^16 identities with 32-byte messages, whole calls and by stage:
      every engine call of the planner between a device synchronisation before and after, by the wall clock.

After one warm-up of every shape: `runs` repetitions, each `reps` calls back to back between two device events, over reps; min, median
and max.  Planner calls: wall clock around a device synchronisation.  Not measured here: the host-pointer entry, more than one device.

    python tools/gt_xor_mask_bench.py [--runs 7] [--reps 20] [--commit ID] [--out profiles/gt_xor_mask.json]
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
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="calls back to back inside one timed window")
    ap.add_argument("--items", type=int, default=1 << 20)
    ap.add_argument("--identities", type=int, default=1 << 16, help="0: skip the planner")
    ap.add_argument("--planner-runs", type=int, default=3)
    ap.add_argument("--commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_xor_mask.json"))
    args = ap.parse_args()
    import torch
    from gopairingbasedcryptography_amd import _build, bf01, bn254 as eng
    _build.build_library()
    eng.init(0)
    dev = torch.device("cuda", 0)
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
    n = args.items
    doc = {"what": "gt_xor_mask beside gt_marshal + torch.bitwise_xor, ragged beside padded, and the bf01 planner by stage, one MI355X",
           "device": torch.cuda.get_device_name(0), "commit": commit, "date": time.strftime("%Y-%m-%d"), "runs": args.runs, "reps": args.reps, "items": n,
           "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
           "timing": "every shape warmed up once; `runs` repetitions, each `reps` calls back to back between two device events, over reps; the legs of one "
                     "comparison alternate inside every repetition; planner calls and their stages: wall clock around a device synchronisation",
           "not_measured": ["the host-pointer entry gpbc_gt_xor_mask", "more than one device"]}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    def timed(legs):
        """{name: stats}: the legs alternate inside every repetition"""
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

    gen = torch.Generator(device=dev)
    gen.manual_seed(2001)
    gt = torch.randint(0, 256, (n, 12, 32), dtype=torch.uint8, device=dev, generator=gen)
    gt[:, :, 31] &= 0x1F                                      # every coefficient below 2^253 < p: canonical Montgomery words, as a GT element's are
    gt = gt.reshape(n, 384)
    copy_src = torch.empty(n * 384 * 2, dtype=torch.uint8, device=dev)
    copy_dst = torch.empty_like(copy_src)

    def rate(rec, moved):
        r = moved / (rec["median_ms"] * 1e-3)
        rec.update({"least_bytes_moved": moved, "bytes_per_s": r, "fraction_of_hbm_peak": r / HBM_PEAK_BYTES_PER_S})

    # ---- (1), (2), (4): rows of one width
    doc["rows"] = []
    for width in (32, 384):
        msgs = torch.randint(0, 256, (n, width), dtype=torch.uint8, device=dev, generator=gen)
        out, work = torch.empty_like(msgs), msgs.clone()
        got, lens = eng.gt_xor_mask(gt, msgs, out=out)
        ref = torch.bitwise_xor(msgs, eng.gt_marshal(gt)[:, :width])
        assert torch.equal(got, ref) and bool((lens == width).all()), "the two routes differ at width %d" % width
        del ref
        moved = n * (32 * ((width + 31) // 32) + 2 * width)   # GT pieces read + message read + output written
        half = moved // 2
        legs = {"gt_xor_mask": lambda: eng.gt_xor_mask(gt, msgs, out=out),
                "gt_xor_mask_in_place": lambda: eng.gt_xor_mask(gt, work, out=work),
                "gt_marshal_then_bitwise_xor": lambda: torch.bitwise_xor(msgs, eng.gt_marshal(gt)[:, :width], out=out),
                "gt_marshal_alone": lambda: eng.gt_marshal(gt),
                "plain_copy_of_the_least_bytes": lambda: copy_dst[:half].copy_(copy_src[:half])}
        rec = timed(legs)
        for name in ("gt_xor_mask", "gt_xor_mask_in_place", "plain_copy_of_the_least_bytes"):
            rate(rec[name], moved)
        rec["gt_marshal_then_bitwise_xor"]["bytes_moved"] = n * (384 + 384 + 384 + 2 * width)      # marshal: 384 in, 384 out; xor: `width` of 384-byte rows (whole lines) + message in + out
        rec.update({"width": width, "items": n,
                    "marshal_route_over_gt_xor_mask": rec["gt_marshal_then_bitwise_xor"]["median_ms"] / rec["gt_xor_mask"]["median_ms"],
                    "gt_xor_mask_over_plain_copy": rec["gt_xor_mask"]["median_ms"] / rec["plain_copy_of_the_least_bytes"]["median_ms"]})
        doc["rows"].append(rec)
        print("width %3d x %d: gt_xor_mask %.3f ms (in place %.3f), gt_marshal + xor %.3f ms (marshal alone %.3f), plain copy of %d MB %.3f ms" % (
            width, n, rec["gt_xor_mask"]["median_ms"], rec["gt_xor_mask_in_place"]["median_ms"], rec["gt_marshal_then_bitwise_xor"]["median_ms"],
            rec["gt_marshal_alone"]["median_ms"], moved >> 20, rec["plain_copy_of_the_least_bytes"]["median_ms"]), flush=True)
        del msgs, out, work
        save()

    # ---- (3): ragged beside padded, and the byte path
    lengths = (np.arange(n, dtype=np.int64) % 64) + 1
    off_host = np.zeros(n + 1, dtype=np.int64)
    off_host[1:] = np.cumsum(lengths)
    total = int(off_host[-1])
    off = torch.from_numpy(off_host).to(dev)
    flat = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=gen)
    flat_out = torch.empty_like(flat)
    padded = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    col = torch.arange(64, device=dev)[None, :] < torch.from_numpy(lengths).to(dev)[:, None]
    padded[col] = flat                                        # row-major: the same bytes, each message at the start of its row
    padded_out = torch.empty_like(padded)
    got, lens = eng.gt_xor_mask(gt, flat, off, out=flat_out)
    ref, _ = eng.gt_xor_mask(gt, padded, out=padded_out)
    assert torch.equal(got, ref[col]) and torch.equal(lens.cpu(), torch.from_numpy(lengths).to(torch.int32)), "ragged and padded differ"
    odd = torch.randint(0, 256, (n, 33), dtype=torch.uint8, device=dev, generator=gen)
    odd_out = torch.empty_like(odd)
    assert torch.equal(eng.gt_xor_mask(gt, odd, out=odd_out)[0], torch.bitwise_xor(odd, eng.gt_marshal(gt)[:, :33]))
    full_off = torch.arange(0, (n + 1) * 384, 384, dtype=torch.int64, device=dev)          # the offset form on messages that all reach every window
    full = torch.randint(0, 256, (n, 384), dtype=torch.uint8, device=dev, generator=gen)
    full_out = torch.empty_like(full)
    assert torch.equal(eng.gt_xor_mask(gt, full.reshape(-1), full_off, out=full_out.reshape(-1))[0].reshape(n, 384), eng.gt_xor_mask(gt, full)[0])
    rec = timed({"ragged_lengths_1_to_64": lambda: eng.gt_xor_mask(gt, flat, off, out=flat_out),
                 "offset_form_all_384": lambda: eng.gt_xor_mask(gt, full.reshape(-1), full_off, out=full_out.reshape(-1)),
                 "rows_of_384": lambda: eng.gt_xor_mask(gt, full, out=full_out),
                 "padded_rows_of_64": lambda: eng.gt_xor_mask(gt, padded, out=padded_out),
                 "rows_of_33": lambda: eng.gt_xor_mask(gt, odd, out=odd_out)})
    pieces = int(((lengths + 31) // 32).sum())
    rate(rec["ragged_lengths_1_to_64"], 32 * pieces + 2 * total + 8 * (n + 1))
    rate(rec["padded_rows_of_64"], n * (64 + 128))
    rate(rec["rows_of_33"], n * (64 + 66))
    rate(rec["offset_form_all_384"], n * (384 * 3 + 8))
    rate(rec["rows_of_384"], n * 384 * 3)
    rec.update({"items": n, "message_bytes": total, "padded_bytes": n * 64,
                "ragged_over_padded": rec["ragged_lengths_1_to_64"]["median_ms"] / rec["padded_rows_of_64"]["median_ms"]})
    doc["ragged"] = rec
    print("ragged 1..64 x %d (%d MB): %.3f ms; padded rows of 64: %.3f ms; rows of 33 (byte path): %.3f ms; offset form, all 384: %.3f ms against rows of 384: %.3f ms" % (
        n, total >> 20, rec["ragged_lengths_1_to_64"]["median_ms"], rec["padded_rows_of_64"]["median_ms"], rec["rows_of_33"]["median_ms"],
        rec["offset_form_all_384"]["median_ms"], rec["rows_of_384"]["median_ms"]), flush=True)
    del full, full_out, full_off, gt, flat, flat_out, padded, padded_out, odd, odd_out, col, copy_src, copy_dst
    torch.cuda.empty_cache()
    save()

    # ---- (5): the planner
    k = args.identities
    if k:
        names = [("user-%d@example.org" % i).encode() for i in range(k)]
        id_off = np.zeros(k + 1, dtype=np.int64)
        id_off[1:] = np.cumsum([len(s) for s in names])
        ids = torch.from_numpy(np.frombuffer(b"".join(names), dtype=np.uint8).copy()).to(dev)
        id_off = torch.from_numpy(id_off).to(dev)
        x = 0x1234567890ABCDEF1234567890ABCDEF % eng.R_ORDER
        g1x = bf01.public_params(eng, x)
        messages = torch.randint(0, 256, (k, 32), dtype=torch.uint8, device=dev, generator=gen)
        r = eng.fr_random(bytes(range(32)), k, stream=0, like=messages)
        qids = bf01.identities_to_g2(eng, ids, id_off)
        sk = bf01.keygen_batch(eng, x, qids=qids)
        q0 = qids[:1].expand(k, 128).contiguous()             # one identity for the one-key Decrypt
        c1, c2, _ = bf01.encrypt_batch(eng, g1x, messages, r, qids=q0)
        back, _ = bf01.decrypt_batch(eng, sk[0], c1, c2)
        assert torch.equal(back, messages), "the round trip does not recover the messages"
        calls = {
            "keygen_batch": lambda e: bf01.keygen_batch(e, x, qids=bf01.identities_to_g2(e, ids, id_off)),
            "encrypt_batch": lambda e: bf01.encrypt_batch(e, g1x, messages, r, qids=bf01.identities_to_g2(e, ids, id_off)),
            "decrypt_batch_one_key": lambda e: bf01.decrypt_batch(e, sk[0], c1, c2),
            "decrypt_batch_key_per_item": lambda e: bf01.decrypt_batch(e, sk, c1, c2),
        }
        plan = {"identities": k, "message_bytes": 32}
        for name, fn in calls.items():
            fn(eng)
            torch.cuda.synchronize()
            whole, stages = [], []
            for _ in range(args.planner_runs):
                t0 = time.perf_counter()
                fn(eng)
                torch.cuda.synchronize()
                whole.append((time.perf_counter() - t0) * 1e3)
                staged = Staged(eng, torch)
                fn(staged)
                stages.append(staged.ms)
            plan[name] = {"whole_call": stats(whole), "stages_median_ms": {s: statistics.median(run[s] for run in stages) for s in stages[0]}}
            print("%s x %d: %.1f ms; %s" % (name, k, plan[name]["whole_call"]["median_ms"],
                                            ", ".join("%s %.2f" % kv for kv in plan[name]["stages_median_ms"].items())), flush=True)
        doc["bf01"] = plan
        save()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
