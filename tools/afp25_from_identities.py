#!/usr/bin/env python3
"""BASELINE config 5 from identities and SRS, measured on one MI355X: writes profiles/afp25_from_identities.json.

  * afp25.decrypt_batches on 2^18 device-resident identities in batches of B = 256 (items/s; warm-up, then the median of RUNS timed
    runs between device events on the stream), and its parts timed the same way: the coefficient kernel, the digest MSM, the
    quotient kernel and the opening MSM chunk by chunk, the pairing part on ready-made openings.  The two polynomial kernels
    are single launches, so the events around their entries are kernel times; bytes written over that time is their achieved
    write bandwidth;
  * the same 64 batches (2^14 items) through the host route — afp25.decrypt_batch(table=...): Python synthetic division per
    identity, host rows into the table's MSM — and through decrypt_batches; the messages of both are compared;
  * fr_mul and fr_inverse on 2^20 HBM-resident elements with their share of the HBM peak (3 x 32 B resp. 2 x 32 B per element);
  * optionally the headline lines of two bench.py runs made back to back on the same box (--bench-before / --bench-after:
    files holding the JSON line), copied in side by side.

    python tools/afp25_from_identities.py [--items 262144] [--runs 5] [--out profiles/afp25_from_identities.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12           # bytes/s, MI355X specification


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 18)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--host-batches", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--bench-before")
    ap.add_argument("--bench-after")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "afp25_from_identities.json"))
    args = ap.parse_args()
    import torch
    import bench_workloads as w
    from gopairingbasedcryptography_amd import _build, afp25, bn254 as eng
    _build.build_library()
    eng.init(0)
    dev = torch.device("cuda", 0)
    n, B = args.items, args.batch
    k = n // B
    inst = w.afp25_instance(eng, B, n, dev)
    table = afp25.srs_table(eng, inst["g1"], w.afp25_srs(eng, inst))
    rows = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in inst["ids"]), dtype=np.uint8).copy()
    ids = torch.from_numpy(rows).to(dev)

    def timed(fn, runs=args.runs, warmup=1):
        """median and all samples, in ms, of fn() between two events on the current stream"""
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

    doc = {"what": "AFP25 batch decryption from device-resident identities and the SRS table (afp25.decrypt_batches), one MI355X",
           "items": n, "B": B, "batches": k, "runs": args.runs, "timing": "median of the runs, device events on the stream, one warm-up"}
    # ---- the whole path
    t_all, s_all, msgs = timed(lambda: afp25.decrypt_batches(eng, table, ids, inst["sk"], inst["C1"], inst["C2"]))
    assert bool((msgs == inst["msgs"]).all()), "decrypt_batches did not recover the messages"
    doc["decrypt_batches"] = {"ms": t_all, "samples_ms": s_all, "items_per_s": n / (t_all * 1e-3)}
    # ---- its parts
    t_roots, s_roots, coeffs = timed(lambda: eng.fr_poly_from_roots(ids, B))
    t_dmsm, _, D = timed(lambda: table.msm(coeffs.reshape(-1)))
    per_batch = B * (B + 1) * 32
    chunk = min(k, max(1, afp25.QUOTIENT_SCRATCH_BYTES // per_batch))
    scratch = torch.empty(chunk * per_batch, dtype=torch.uint8, device=dev)
    okbuf = torch.empty(chunk * B, dtype=torch.uint8, device=dev)
    cf = coeffs.reshape(-1)
    t_q = t_m = 0.0
    q_samples = []
    for lo in range(0, k, chunk):
        m = min(chunk, k - lo)
        quot = lambda: eng.fr_poly_quotients(cf[lo * (B + 1) * 32:(lo + m) * (B + 1) * 32], ids[lo * B * 32:(lo + m) * B * 32], B, B + 1,
                                             out=scratch[:m * per_batch], ok=okbuf[:m * B])
        tq, sq, (q, ok) = timed(quot)
        tm, _, _ = timed(lambda: table.msm(q))
        t_q += tq
        t_m += tm
        q_samples.append(sq)
    t_pair, s_pair, _ = timed(lambda: afp25.decrypt_batch_arrays(eng, inst["D"], inst["pi"], inst["sk"], inst["C1"], inst["C2"]))
    doc["split_ms"] = {"k_fr_poly_from_roots": t_roots, "digest_msm": t_dmsm, "k_fr_poly_quotients": t_q, "opening_msm": t_m, "pairing_part": t_pair,
                       "sum": t_roots + t_dmsm + t_q + t_m + t_pair, "quotient_chunks": (k + chunk - 1) // chunk, "msm_terms": n * (B + 1) + k * (B + 1)}
    doc["pairing_part_items_per_s"] = n / (t_pair * 1e-3)
    doc["kernels"] = {
        "k_fr_poly_from_roots": {"ms": t_roots, "samples_ms": s_roots, "bytes_written": k * (B + 1) * 32, "write_GBps": k * (B + 1) * 32 / (t_roots * 1e-3) / 1e9,
                                 "fr_products": k * B * (B + 3) // 2},
        "k_fr_poly_quotients": {"ms": t_q, "chunk_samples_ms": q_samples, "bytes_written": n * (B + 1) * 32, "write_GBps": n * (B + 1) * 32 / (t_q * 1e-3) / 1e9,
                                "share_of_hbm_peak": n * (B + 1) * 32 / (t_q * 1e-3) / HBM_PEAK, "fr_products": n * (B + 1)},
    }
    del scratch, okbuf
    # ---- the host route on the first batches, and the new path on the same items
    hb = min(args.host_batches, k)
    srs = w.afp25_srs(eng, inst)
    host = {key: inst[key][:hb * B].cpu().numpy() for key in ("D", "sk", "C1", "C2")}
    t0 = time.perf_counter()
    got_host = []
    for b in range(hb):
        bid = inst["ids"][b * B:(b + 1) * B]
        f = afp25.poly_from_roots(bid)
        items = [(bid[t], host["C1"][b * B + t], host["C2"][b * B + t]) for t in range(B)]
        got_host.append(afp25.decrypt_batch(eng, inst["g1"], srs, host["D"][b * B], f, host["sk"][b * B], items, table=table, identities=bid))
    t_host = time.perf_counter() - t0
    got_host = np.concatenate(got_host)
    sub = lambda x, width: x.reshape(n, -1)[:hb * B].contiguous()
    t_new, s_new, got_new = timed(lambda: afp25.decrypt_batches(eng, table, ids[:hb * B * 32], sub(inst["sk"], 64), sub(inst["C1"], 384), sub(inst["C2"], 384)))
    same = bool((got_new.cpu().numpy() == got_host).all()) and bool((got_new == inst["msgs"][:hb * B]).all())
    assert same, "the host route and decrypt_batches disagree"
    doc["host_route_vs_new"] = {"items": hb * B, "host_route": "afp25.decrypt_batch(table=...) per batch: Python poly_from_roots / quotient_by_root, host rows into the table's MSM (digest given)",
                                "host_route_s": t_host, "host_route_items_per_s": hb * B / t_host, "decrypt_batches_ms": t_new, "decrypt_batches_samples_ms": s_new,
                                "decrypt_batches_items_per_s": hb * B / (t_new * 1e-3), "speedup": t_host / (t_new * 1e-3), "messages_equal": same}
    # ---- elementwise at 2^20
    m = 1 << 20
    rng = np.random.default_rng(5)
    a = torch.from_numpy(rng.integers(0, 256, size=m * 32, dtype=np.uint8)).to(dev)
    b = torch.from_numpy(rng.integers(0, 256, size=m * 32, dtype=np.uint8)).to(dev)
    out = torch.empty((m, 32), dtype=torch.uint8, device=dev)
    t_mul, s_mul, _ = timed(lambda: eng.fr_mul(a, b, out=out), runs=max(args.runs, 9), warmup=2)
    t_inv, s_inv, _ = timed(lambda: eng.fr_inverse(a, out=out), runs=max(args.runs, 9), warmup=2)
    doc["elementwise_2_20"] = {
        "fr_mul": {"ms": t_mul, "samples_ms": s_mul, "bytes": 96 * m, "GBps": 96 * m / (t_mul * 1e-3) / 1e9, "share_of_hbm_peak": 96 * m / (t_mul * 1e-3) / HBM_PEAK},
        "fr_inverse": {"ms": t_inv, "samples_ms": s_inv, "bytes": 64 * m, "GBps": 64 * m / (t_inv * 1e-3) / 1e9, "share_of_hbm_peak": 64 * m / (t_inv * 1e-3) / HBM_PEAK},
        "hbm_peak_Bps": HBM_PEAK}
    for key, path in (("bench_py_parent", args.bench_before), ("bench_py_this", args.bench_after)):
        if path and os.path.exists(path):
            lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
            line = json.loads(lines[-1]) if lines else {}
            doc[key] = {f: line.get(f) for f in ("metric", "value", "unit", "steps", "warmup", "ms_per_step")}
    table.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({key: doc[key] for key in ("decrypt_batches", "split_ms", "host_route_vs_new", "elementwise_2_20")}, indent=1))


if __name__ == "__main__":
    main()
