#!/usr/bin/env python3
"""Waters11 CP-ABE batched decryption measured on one MI355X: writes profiles/waters11_decrypt.json.

  (a) fr_lsss_weights alone on HBM-resident inputs — 2^16 systems of 16 x 16 (the policies of (b), a matrix per system) and 2^10 dense
      systems of 64 x 64 with every row held — as systems per second;
  (b) waters11.decrypt_batch on one key against 2^14 ciphertexts whose 16-row policies cycle through AND chains, a threshold and an
      AND / OR formula (every 64th one unsatisfied), whole and stage by stage: solve, scalar multiplications, additions,
      multi-pairing, GT;
  (c) the first 2^12 of those ciphertexts through waters11.decrypt_batch_host_weights — the weights from lw11.reconstruction_weights,
      one elimination in Python integers per ciphertext, then the identical engine calls — against decrypt_batch on the same
      ciphertexts, in the same call sequence; the messages of both are compared.

Warm-up, then the median of RUNS timed runs between device events on the stream.  The instance is tests/waters11_fixture.py's.

    python tools/waters11_decrypt.py [--items 16384] [--host-items 4096] [--runs 5] [--commit ID] [--out profiles/waters11_decrypt.json]
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
    ap.add_argument("--items", type=int, default=1 << 14)
    ap.add_argument("--host-items", type=int, default=1 << 12)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "waters11_decrypt.json"))
    args = ap.parse_args()
    import torch
    from waters11_fixture import Instance, at_size_policies
    from gopairingbasedcryptography_amd import _build, bn254 as eng, waters11
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

    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    doc = {"what": "Waters11 CP-ABE batched decryption (waters11.decrypt_batch) and fr_lsss_weights, one MI355X",
           "device": torch.cuda.get_device_name(0), "commit": commit, "date": time.strftime("%Y-%m-%d"), "runs": args.runs,
           "timing": "median of the runs, device events on the stream, one warm-up"}
    n, R = args.items, 16
    pols, key_attrs = at_size_policies(n)
    pad = waters11.pad_policies(pols, rows=R)
    held = waters11.held_mask(pad.rho, key_attrs)
    # ---- (a) the kernel alone
    solves = []
    k16 = 1 << 16
    reps = (k16 + n - 1) // n
    m16, h16 = put(np.tile(pad.matrix.reshape(n, -1), (reps, 1))[:k16]).reshape(-1), put(np.tile(held, (reps, 1))[:k16]).reshape(-1)
    w16, ok16 = torch.empty((k16, R, 32), dtype=torch.uint8, device=dev), torch.empty((k16,), dtype=torch.uint8, device=dev)
    t, smp, _ = timed(lambda: eng.fr_lsss_weights(m16, R, pad.cols, h16, out=w16, ok_out=ok16))
    solves.append({"shape": "2^16 x (16 x %d), the policies of the decrypt" % pad.cols, "systems": k16, "rows": R, "cols": pad.cols, "ms": t, "samples_ms": smp,
                   "systems_per_s": k16 / (t * 1e-3), "ok": int(ok16.sum())})
    rng = np.random.default_rng(2011)
    k64 = 1 << 10
    m64 = torch.from_numpy(rng.integers(0, 256, size=k64 * 64 * 64 * 32, dtype=np.uint8)).to(dev)
    h64 = torch.ones(k64 * 64, dtype=torch.uint8, device=dev)
    t, smp, (_, ok64) = timed(lambda: eng.fr_lsss_weights(m64, 64, 64, h64))
    solves.append({"shape": "2^10 x (64 x 64), dense random, every row held", "systems": k64, "rows": 64, "cols": 64, "ms": t, "samples_ms": smp,
                   "systems_per_s": k64 / (t * 1e-3), "ok": int(ok64.sum()), "fr_mul2_per_system": 64 * 63 * 65, "fr_mul2_per_s": k64 * 64 * 63 * 65 / (t * 1e-3)})
    del m16, h16, w16, ok16, m64, h64
    doc["fr_lsss_weights"] = solves
    # ---- (b) the decrypt
    inst = Instance(eng, key_attrs, pols, rows=R, dev=dev, tag="m")
    doc["shape"] = {"ciphertexts": n, "rows_per_policy": R, "cols": pad.cols, "key_attributes": len(key_attrs), "unsatisfied": n // 64,
                    "policies": "AND chain of 16 / 8 of 16 / (8 and) or (8 and) / AND chain of 5 padded to 16, in turn"}
    whole = lambda: waters11.decrypt_batch(eng, inst.key, pad, inst.c, inst.c_prime, inst.cx, inst.dx)
    t0 = time.perf_counter()
    msgs, ok = whole()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    good = ok.bool()
    assert int((~good).sum()) == n // 64 and bool((msgs[good] == inst.msgs.reshape(n, 384)[good]).all()) and not bool(msgs[~good].any())
    t_all, s_all, _ = timed(whole)
    # the stages on the planner's own intermediates
    dm, dh = put(pad.matrix).reshape(-1), put(held).reshape(-1)
    t_solve, _, (w, _) = timed(lambda: eng.fr_lsss_weights(dm, R, pad.cols, dh))
    nw = eng.fr_neg(w.reshape(-1))
    attrs = sorted(inst.key[2])
    comp = np.zeros((len(attrs) + 1, 64), dtype=np.uint8)
    for i, a in enumerate(attrs):
        comp[i] = inst.key[2][a]
    gathered = put(comp).index_select(0, put(waters11.key_index(pad.rho, attrs).reshape(-1))).reshape(-1)
    cx = inst.cx.reshape(-1)
    t_smul, _, (S, T) = timed(lambda: (eng.g1_scalar_mul(cx, nw.reshape(-1)), eng.g1_scalar_mul(gathered, nw.reshape(-1))))

    def additions():
        s, m = S.reshape(n, R, 64), R
        while m > 1:
            h = m // 2
            s = eng.g1_add(s[:, :h].contiguous().reshape(-1), s[:, h:2 * h].contiguous().reshape(-1)).reshape(n, h, 64)
            m = h
        return s
    t_add, _, Ssum = timed(additions)
    P = torch.cat([put(np.broadcast_to(inst.key[0].reshape(1, 1, 64), (n, 1, 64))), Ssum.reshape(n, 1, 64), T.reshape(n, R, 64)], 1).contiguous().reshape(-1)
    Q = torch.cat([inst.c_prime.reshape(n, 1, 128), put(np.broadcast_to(inst.key[1].reshape(1, 1, 128), (n, 1, 128))), inst.dx.reshape(n, R, 128)], 1).contiguous().reshape(-1)
    seg = np.arange(0, (R + 2) * n + 1, R + 2, dtype=np.uint64)
    t_pair, _, E = timed(lambda: eng.multi_pair(P, Q, seg))
    c = inst.c.reshape(-1)
    t_gt, _, _ = timed(lambda: eng.gt_div(c, E.reshape(-1)))
    stages = {"solve": t_solve, "scalar_mul": t_smul, "additions": t_add, "multi_pair": t_pair, "gt": t_gt}
    doc["decrypt_batch"] = {"ms": t_all, "samples_ms": s_all, "ciphertexts_per_s": n / (t_all * 1e-3), "first_call_wall_s": wall,
                            "whole_includes": "the numpy mask and index table, the upload of the padded matrices (%d MB) and the gathers, besides the stages below" % (pad.matrix.nbytes >> 20),
                            "split_ms": dict(stages, sum=sum(stages.values())), "largest_device_stage": max(stages, key=stages.get),
                            "solve_share_of_multi_pair": t_solve / t_pair, "pairs_per_ciphertext": R + 2, "scalar_muls": 2 * n * R}
    # ---- (c) the host-weights route on the first ciphertexts, same call sequence
    hn = min(args.host_items, n)
    sub = pols[:hn]
    part = lambda a, width, per: a.reshape(-1, width)[:hn * per].contiguous()
    sargs = (part(inst.c, 384, 1), part(inst.c_prime, 128, 1), part(inst.cx, 64, R), part(inst.dx, 128, R))
    t0 = time.perf_counter()
    got_host, ok_host = waters11.decrypt_batch_host_weights(eng, inst.key, sub, *sargs)
    torch.cuda.synchronize()
    t_host = time.perf_counter() - t0
    from gopairingbasedcryptography_amd import lw11
    t0 = time.perf_counter()
    ks = set(key_attrs)
    for m, rho in sub:
        lw11.reconstruction_weights(m, rho, ks)
    t_py = time.perf_counter() - t0
    spad = waters11.pad_policies(sub, rows=R)
    t_new, s_new, (got_new, ok_new) = timed(lambda: waters11.decrypt_batch(eng, inst.key, spad, *sargs))
    same = bool((got_new == got_host).all()) and bool((ok_new == ok_host).all())
    assert same, "the host-weights route and decrypt_batch disagree"
    sm, sh = put(spad.matrix).reshape(-1), put(waters11.held_mask(spad.rho, key_attrs)).reshape(-1)
    t_solve_sub, _, _ = timed(lambda: eng.fr_lsss_weights(sm, R, spad.cols, sh))
    doc["host_weights_vs_device"] = {
        "ciphertexts": hn, "host_route": "decrypt_batch_host_weights: lw11.reconstruction_weights per ciphertext (Python integers), uploaded; then the engine calls of decrypt_batch",
        "host_route_total_s": t_host, "python_eliminations_s": t_py, "eliminations_share_of_host_route": t_py / t_host,
        "decrypt_batch_ms": t_new, "decrypt_batch_samples_ms": s_new, "device_solve_ms": t_solve_sub,
        "solve_stage_ratio": t_py / (t_solve_sub * 1e-3), "whole_ratio": t_host / (t_new * 1e-3), "messages_equal": same}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
