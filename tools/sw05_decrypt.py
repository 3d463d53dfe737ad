#!/usr/bin/env python3
"""SW05 fuzzy IBE batched decryption measured on one MI355X: writes profiles/sw05_decrypt.json.

  (a) fr_lagrange_basis alone on HBM-resident inputs at three shapes — 2^16 rows of B = m = 16, 2^12 rows of 64, and the shared-set
      form of computeT (2^16 values of x, 17 nodes over a 17-element set) — as products per second (2 B + 4 per output) and against
      fr_inverse on as many elements as there are outputs: the kernel is that inversion, shared by four outputs, plus its products;
  (b) sw05.decrypt_batch and sw05.decrypt_batch_large on 2^16 ciphertexts with d = 16, whole and stage by stage (Lagrange, scalar
      multiplications, multi-pairing, GT);
  (c) the first 2^12 of those ciphertexts through the route the parent commit allows — the coefficients in Python integers (one
      modular inversion per coefficient, as bsw07.lagrange_at_zero computes them), uploaded, then the identical engine calls — against
      the planner on the same ciphertexts; the messages of both are compared.
  (d) optionally the headline lines of bench.py runs on the parent commit's library and on this tree's, alternating on the same box
      (--bench-parent / --bench-this: files holding one JSON line per run), copied in side by side.

Warm-up, then the median of RUNS timed runs between device events on the stream.  The instance is tests/sw05_fixture.py's.

    python tools/sw05_decrypt.py [--items 65536] [--runs 5] [--commit ID] [--out profiles/sw05_decrypt.json]
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

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 16)
    ap.add_argument("--host-items", type=int, default=1 << 12)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--commit")
    ap.add_argument("--bench-parent")
    ap.add_argument("--bench-this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sw05_decrypt.json"))
    args = ap.parse_args()
    import torch
    from sw05_fixture import Instance, at_size_attributes, kbytes
    from gopairingbasedcryptography_amd import _build, bn254 as eng, sw05
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

    doc = {"what": "SW05 fuzzy IBE batched decryption (sw05.decrypt_batch / decrypt_batch_large) and fr_lagrange_basis, one MI355X",
           "device": torch.cuda.get_device_name(0), "commit": commit, "date": time.strftime("%Y-%m-%d"), "runs": args.runs,
           "timing": "median of the runs, device events on the stream, one warm-up"}
    # ---- (a) the kernel alone
    rng = np.random.default_rng(2005)
    rand = lambda n: torch.from_numpy(rng.integers(0, 256, size=n * 32, dtype=np.uint8)).to(dev)
    shapes = []
    for label, k, B, m, shared in (("2^16 x 16", 1 << 16, 16, 16, False), ("2^12 x 64", 1 << 12, 64, 64, False), ("shared set 17, 17 nodes, 2^16 x", 1 << 16, 17, 17, True)):
        if shared:
            s, nd, x = torch.from_numpy(kbytes(range(1, 18)).copy()).to(dev), torch.from_numpy(kbytes(range(17)).copy()).to(dev), rand(k)
        else:
            s, nd, x = rand(k * B), None, None
        out = torch.empty((k, m, 32), dtype=torch.uint8, device=dev)
        t, smp, _ = timed(lambda: eng.fr_lagrange_basis(s, B, nd, m if nd is not None else None, x, out=out))
        flat = out.reshape(-1, 32)
        t_inv, smp_inv, _ = timed(lambda: eng.fr_inverse(flat, out=torch.empty_like(flat)))
        products = k * m * (2 * B + 4)
        shapes.append({"shape": label, "rows": k, "B": B, "m": m, "shared_set": shared, "ms": t, "samples_ms": smp, "outputs_per_s": k * m / (t * 1e-3),
                       "fr_products": products, "products_per_s": products / (t * 1e-3),
                       "fr_inverse_same_count_ms": t_inv, "fr_inverse_samples_ms": smp_inv, "fr_inverse_share_of_time": t_inv / t})
    doc["fr_lagrange_basis"] = shapes
    # ---- (b) the two decrypts
    n, a, n_key, d = args.items, 24, 32, 16
    key_attrs, cts = at_size_attributes(n, a, n_key, d, every=64)
    doc["shape"] = {"ciphertexts": n, "attributes_per_ciphertext": a, "key_attributes": n_key, "d": d, "below_threshold": n // 64}
    for large in (False, True):
        name = "decrypt_batch_large" if large else "decrypt_batch"
        inst = Instance(eng, d, key_attrs, cts, n_univ=a if large else None, dev=dev, tag="m")
        if large:
            whole = lambda c=cts, i=inst: sw05.decrypt_batch_large(eng, i.key, d, c, i.E, i.e_pp, i.e_prime)
        else:
            whole = lambda c=cts, i=inst: sw05.decrypt_batch(eng, i.key, d, c, i.E, i.e_prime)
        t0 = time.perf_counter()
        msgs, ok = whole()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        good = ok.bool()
        assert int((~good).sum()) == n // 64 and bool((msgs[good] == inst.msgs.reshape(n, 384)[good]).all()) and not bool(msgs[~good].any()), name
        t_all, s_all, _ = timed(whole)
        # the stages on the planner's own intermediates
        p = sw05._Plan(eng, inst.key[0], d, cts, inst.E, inst.e_prime)
        sets = torch.from_numpy(kbytes(cts[t][q] for t in p.good for q in p.ct_pos[t]).copy()).to(dev)
        t_lag, _, delta = timed(lambda: eng.fr_lagrange_basis(sets, d))
        delta = delta.reshape(p.ng, d, 32)
        if large:
            epp = p.rows(inst.e_pp.reshape(n, 64)).reshape(p.ng, 1, 64).expand(p.ng, d, 64)
            bases = torch.cat([p.key_rows(inst.key[1], 64), epp], 1).contiguous().reshape(-1)
            neg = lambda: torch.cat([delta, eng.fr_neg(delta.reshape(-1)).reshape(p.ng, d, 32)], 1).contiguous().reshape(-1)
            t_smul, _, P = timed(lambda: eng.g1_scalar_mul(bases, neg()))
            Q = torch.cat([p.ct_rows(), p.key_rows(inst.key[2], 128)], 1).contiguous().reshape(-1)
            pairs = 2 * d
        else:
            bases = p.key_rows(inst.key[1], 64).contiguous().reshape(-1)
            t_smul, _, P = timed(lambda: eng.g1_scalar_mul(bases, delta.reshape(-1)))
            Q = p.ct_rows().contiguous().reshape(-1)
            pairs = d
        t_pair, _, den = timed(lambda: eng.multi_pair(P.reshape(-1), Q, p.seg(pairs)))
        ep = p.rows(p.e_prime)
        t_gt, _, _ = timed(lambda: (eng.gt_mul if large else eng.gt_div)(ep, den))
        doc[name] = {"ms": t_all, "samples_ms": s_all, "ciphertexts_per_s": n / (t_all * 1e-3), "first_call_wall_s": wall,
                     "whole_includes": "host selection of the common attributes (Python) and the gathers, besides the stages below",
                     "split_ms": {"lagrange": t_lag, "scalar_mul": t_smul, "multi_pair": t_pair, "gt": t_gt, "sum": t_lag + t_smul + t_pair + t_gt},
                     "lagrange_share_of_multi_pair": t_lag / t_pair, "pairs_per_ciphertext": pairs, "scalar_muls": p.ng * pairs}
        # ---- (c) the host route of the parent commit on the first ciphertexts
        if not large:
            hn = min(args.host_items, n)
            sub = cts[:hn]
            t0 = time.perf_counter()
            kp, cp, okh = sw05.select_common(inst.key[0], sub, d)
            gd = np.nonzero(okh)[0]
            t_sel = time.perf_counter() - t0
            t0 = time.perf_counter()
            coeff = []
            for t in gd:
                S = [sub[t][q] % R for q in cp[t]]
                for i in S:
                    num = den_ = 1
                    for j in S:
                        if j != i:
                            num, den_ = num * (-j) % R, den_ * (i - j) % R
                    coeff.append(num * pow(den_, -1, R) % R)
            host_delta = kbytes(coeff)
            t_py = time.perf_counter() - t0
            E_sub, ep_sub = inst.E[:hn].contiguous(), inst.e_prime.reshape(n, 384)[:hn].contiguous()
            idx = torch.as_tensor((gd[:, None] * a + cp[gd]).reshape(-1), dtype=torch.long, device=dev)
            gsel = torch.as_tensor(gd, dtype=torch.long, device=dev)
            kb = torch.from_numpy(np.ascontiguousarray(np.asarray(inst.key[1]).reshape(-1, 64)[kp[gd].reshape(-1)])).to(dev).reshape(-1)

            def host_route():
                dl = torch.from_numpy(host_delta.copy()).to(dev)
                Ph = eng.g1_scalar_mul(kb, dl)
                dn = eng.multi_pair(Ph.reshape(-1), E_sub.reshape(-1, 128).index_select(0, idx).reshape(-1), np.arange(0, d * len(gd) + 1, d, dtype=np.uint64))
                return eng.gt_div(ep_sub.index_select(0, gsel).contiguous(), dn)
            t_eng, s_eng, got_host = timed(host_route)
            t_new, s_new, (got_new, ok_new) = timed(lambda: sw05.decrypt_batch(eng, inst.key, d, sub, E_sub, ep_sub))
            same = bool((got_new[gsel] == got_host).all()) and bool((got_host == inst.msgs.reshape(n, 384)[:hn][gsel]).all())
            assert same, "the host route and decrypt_batch disagree"
            t_lag_sub, _, _ = timed(lambda: eng.fr_lagrange_basis(torch.from_numpy(kbytes(sub[t][q] for t in gd for q in cp[t]).copy()).to(dev), d))
            doc["host_route_vs_new"] = {
                "ciphertexts": hn, "host_route": "coefficients in Python integers (one modular inversion and 2 (d - 1) products each), uploaded; then g1_scalar_mul, multi_pair, gt_div as the planner calls them",
                "python_lagrange_s": t_py, "python_select_common_s": t_sel, "engine_calls_ms": t_eng, "engine_calls_samples_ms": s_eng,
                "host_route_total_s": t_py + t_sel + t_eng * 1e-3, "lagrange_share_of_host_route": t_py / (t_py + t_sel + t_eng * 1e-3),
                "decrypt_batch_ms": t_new, "decrypt_batch_samples_ms": s_new, "device_lagrange_ms": t_lag_sub,
                "lagrange_stage_ratio": t_py / (t_lag_sub * 1e-3), "whole_ratio": (t_py + t_sel + t_eng * 1e-3) / (t_new * 1e-3), "messages_equal": same}
        del inst
        eng.release_workspaces()
    for key, path in (("bench_py_parent", args.bench_parent), ("bench_py_this", args.bench_this)):
        if path and os.path.exists(path):
            runs = [json.loads(ln) for ln in open(path).read().splitlines() if ln.startswith("{")]
            doc[key] = [{f: r.get(f) for f in ("metric", "value", "unit", "steps", "warmup", "ms_per_step")} for r in runs]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
