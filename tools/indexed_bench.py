"""Indexed sums over fixed-base tables and LSSS share generation (gpbc_fixed_base_indexed_dev, gpbc_fr_lsss_shares_dev:
include/gpbc_bn254_indexed.h) on HBM-resident data against the routes the engine had before them to the same bytes, and the planners
built on them:

  * FixedBase.indexed at 2^16 x 256 outputs — G1, one term, 256 periodic index rows over 256 bases (the leaves of BSW07); G1, two terms,
    an index row per output over 257 bases (Waters11 C_x) — and at 2^14 x 16 outputs for G2, two terms, 16 periodic rows over 17 bases
    (LW11 c3x), each against g1 / g2_scalar_mul on the expanded (gathered) bases plus g1 / g2_add for the second term;
  * fr_lsss_shares at 2^16 x (16 x 15) and 2^12 x (64 x 64), one matrix for all and a matrix per item;
  * bsw07.encrypt_batch at 2^16 x 256 leaves with and without tables, waters11.encrypt_batch at 2^14 ciphertexts of 16-row policies,
    lw11.encrypt_batch at 2^14 x 16 rows.
Seeded inputs; the legs of a comparison alternate inside one repetition loop; the output bytes of the routes are compared before any
time is reported; device events.  One process, one device.  The lane order of the periodic cases is the library's: run the tool
again with GPBC_LIB_PATH naming a build with -DGPBC_FBINDEX_GROUP_MIN=SIZE_MAX (the natural order) and --only-indexed for the A/B.
Writes one JSON document (profiles/indexed_fixed_base.json records a run), rewritten after every section.

    python tools/indexed_bench.py [--reps 3] [--log-n 16] [--out FILE] [--only-indexed] [--skip-planners]"""
import argparse
import datetime
import json
import os
import statistics
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopairingbasedcryptography_amd import _lib, bn254, bsw07, lw11, waters11  # noqa: E402
from gopairingbasedcryptography_amd._buffers import R_ORDER as R  # noqa: E402


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def stats(ts):
    return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts), "all_ms": ts}


def alternate(legs, reps):
    """every leg warmed up once, then `reps` rounds of all legs in turn; {name: stats}"""
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            ts[name].append(timed(fn))
    return {name: stats(t) for name, t in ts.items()}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rand_scalars(rng, *shape):
    """uniform 256-bit values: every window digit non-zero 255 times in 256, as for a reduced scalar"""
    return dev(rng.integers(0, 256, size=shape + (32,), dtype=np.uint8))


def points(g2, n, tag):
    ks = rand_scalars(np.random.default_rng(zlib.crc32(tag.encode())), n)
    return (bn254.g2_scalar_mul_base if g2 else bn254.g1_scalar_mul_base)(ks.reshape(-1)).reshape(n, 128 if g2 else 64)


def indexed_section(name, g2, nbase, index, terms, n, reps, rng):
    """FixedBase.indexed against scalar_mul on the gathered bases (+ add for the second term); bytes compared first"""
    width = 128 if g2 else 64
    mul, add = (bn254.g2_scalar_mul, bn254.g2_add) if g2 else (bn254.g1_scalar_mul, bn254.g1_add)
    bases = points(g2, nbase, name)
    table = bn254.FixedBase(bases, g2=g2)
    k = rand_scalars(rng, n, terms)
    idx = dev(index.astype(np.int32))
    P = index.shape[0]
    sel = torch.from_numpy(index.astype(np.int64)).cuda()                       # [P, terms]
    gathered = [bases[sel[:, t]].unsqueeze(0).expand(n // P, P, width).reshape(-1).contiguous() for t in range(terms)]
    cols = [k[:, t].contiguous().reshape(-1) for t in range(terms)]
    out = {}

    def indexed():
        out["indexed"] = table.indexed(idx, k.reshape(-1), terms=terms)[0]

    def composed():
        acc = mul(gathered[0], cols[0])
        for t in range(1, terms):
            acc = add(acc, mul(gathered[t], cols[t]))
        out["composed"] = acc
    indexed(); composed()
    torch.cuda.synchronize()
    same = bool(torch.equal(out["indexed"].reshape(-1), out["composed"].reshape(-1)))
    res = alternate({"indexed": indexed, "scalar_mul_expanded": composed}, reps)
    table.close()
    mults = n * terms
    return {"group": "G2" if g2 else "G1", "nbase": nbase, "terms": terms, "outputs": n, "index_rows": P, "same_bytes": same, **res,
            "indexed_Mmul_per_s": mults / res["indexed"]["median_ms"] / 1e3, "scalar_mul_Mmul_per_s": mults / res["scalar_mul_expanded"]["median_ms"] / 1e3,
            "speedup": res["scalar_mul_expanded"]["median_ms"] / res["indexed"]["median_ms"]}


def shares_section(rows, cols, k, per_item, reps, rng):
    m = rand_scalars(rng, k if per_item else 1, rows, cols)
    v = rand_scalars(rng, k, cols)
    res = alternate({"fr_lsss_shares": lambda: bn254.fr_lsss_shares(m.reshape(-1), v.reshape(-1), rows, cols)}, reps)
    # spot check against Python integers
    got = bn254.fr_lsss_shares(m.reshape(-1), v.reshape(-1), rows, cols)[:2].cpu().numpy()
    ints = lambda t: [int.from_bytes(r.tobytes(), "little") for r in t.cpu().numpy().reshape(-1, 32)]
    mi, vi = ints(m[:2 if per_item else 1]), ints(v[:2])
    want = [sum(mi[(j if per_item else 0) * rows * cols + x * cols + c] * vi[j * cols + c] for c in range(cols)) % R for j in range(2) for x in range(rows)]
    ok = [int.from_bytes(r.tobytes(), "little") for r in got.reshape(-1, 32)] == want
    return {"rows": rows, "cols": cols, "k": k, "matrix": "per item" if per_item else "shared", "checked": ok, **res,
            "Mproducts_per_s": k * rows * cols / res["fr_lsss_shares"]["median_ms"] / 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-indexed", action="store_true")
    ap.add_argument("--skip-planners", action="store_true")
    args = ap.parse_args()
    bn254.init(0)
    rng = np.random.default_rng(2011)
    n16, n14 = 1 << args.log_n, 1 << max(args.log_n - 2, 0)
    doc = {"tool": "tools/indexed_bench.py", "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "library": os.path.relpath(_lib.LIB_PATH, ROOT),
           "reps": args.reps, "log_n": args.log_n, "indexed": {}, "fr_lsss_shares": [], "planners": {}}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
    # ---- A: the primitives
    doc["indexed"]["g1_terms1_periodic_256rows_256bases"] = indexed_section("bsw07", False, 256, np.arange(256).reshape(256, 1), 1, n16 * 256, args.reps, rng)
    save()
    idx = np.stack([np.zeros(n16 * 256, dtype=np.int64), 1 + rng.integers(0, 256, size=n16 * 256)], 1)
    doc["indexed"]["g1_terms2_per_output_257bases"] = indexed_section("waters11", False, 257, idx, 2, n16 * 256, args.reps, rng)
    del idx
    save()
    idx = np.stack([1 + np.arange(16), np.zeros(16, dtype=np.int64)], 1)
    doc["indexed"]["g2_terms2_periodic_16rows_17bases"] = indexed_section("lw11", True, 17, idx, 2, n14 * 16, args.reps, rng)
    save()
    torch.cuda.empty_cache()
    if args.only_indexed:
        print(json.dumps(doc["indexed"]))
        return
    for rows, cols, k in ((16, 15, n16), (64, 64, 1 << max(args.log_n - 4, 0))):
        for per_item in (False, True):
            doc["fr_lsss_shares"].append(shares_section(rows, cols, k, per_item, args.reps, rng))
    save()
    if args.skip_planners:
        print(json.dumps(doc))
        return
    # ---- B: the planners
    e_alpha = np.asarray(bn254.pair(*bn254.generators())).reshape(384)
    # BSW07, 256-of-256, with and without tables
    tree = bsw07.Threshold(256, *[bsw07.Leaf(i) for i in range(256)])
    plan = bsw07.share_plan(tree)
    h1p = points(False, 256, "h1").cpu().numpy()
    h1 = {i: h1p[i] for i in range(256)}
    hpt = points(False, 1, "beta").cpu().numpy().reshape(64)
    msgs = bn254.gt_exp(dev(np.tile(e_alpha, (n16, 1))).reshape(-1), rand_scalars(rng, n16).reshape(-1)).reshape(n16, 384)
    s, q = rand_scalars(rng, n16), rand_scalars(rng, n16, 255)
    outs = {}
    legs = {"tables=False": lambda: outs.__setitem__("a", bsw07.encrypt_batch(bn254, plan, hpt, e_alpha, h1, msgs, s, q)),
            "tables=True": lambda: outs.__setitem__("b", bsw07.encrypt_batch(bn254, plan, hpt, e_alpha, h1, msgs, s, q, tables=True))}
    res = alternate(legs, args.reps)
    doc["planners"]["bsw07_encrypt_256_leaves"] = {"ciphertexts": n16, "same_bytes": all(bool(torch.equal(a, b)) for a, b in zip(outs["a"], outs["b"])), **res,
                                                   "speedup": res["tables=False"]["median_ms"] / res["tables=True"]["median_ms"], "note": "tables=True includes building and freeing the 256-base table"}
    del outs, msgs, s, q
    torch.cuda.empty_cache()
    save()
    # Waters11: 2^14 ciphertexts of the 16-row policies
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
    import waters11_fixture as wf
    import lw11_fixture as lf
    policies, key_attrs = wf.at_size_policies(n14)
    universe = sorted(set(key_attrs) | {u for _, rho in policies[:128] for u in rho})
    hp = points(False, len(universe), "w11h").cpu().numpy()
    h = {u: hp[i] for i, u in enumerate(universe)}
    g1a = points(False, 1, "w11a").cpu().numpy().reshape(64)
    pad = waters11.pad_policies(policies)
    msgs = bn254.gt_exp(dev(np.tile(e_alpha, (n14, 1))).reshape(-1), rand_scalars(rng, n14).reshape(-1)).reshape(n14, 384)
    s, v, r = rand_scalars(rng, n14), rand_scalars(rng, n14, pad.cols - 1), rand_scalars(rng, n14, pad.rows)
    table = waters11.encrypt_table(bn254, g1a, h)
    res = alternate({"encrypt_batch (table built once)": lambda: waters11.encrypt_batch(bn254, g1a, e_alpha, h, pad, msgs, s, v, r, table=table),
                     "encrypt_batch (table built per call)": lambda: waters11.encrypt_batch(bn254, g1a, e_alpha, h, pad, msgs, s, v, r)}, args.reps)
    table.close()
    doc["planners"]["waters11_encrypt_at_size_policies"] = {"ciphertexts": n14, "rows": pad.rows, "cols": pad.cols, "universe": len(universe), **res}
    save()
    # LW11: 2^14 ciphertexts x 16 rows (8 of 16 as Shamir rows)
    m, rho = lf.threshold_policy(8, 16)
    ea = bn254.gt_exp(dev(np.tile(e_alpha, (16, 1))).reshape(-1), rand_scalars(rng, 16).reshape(-1)).reshape(16, 384).cpu().numpy()
    gy = points(True, 16, "lw11y").cpu().numpy()
    egg, g2y = {u: ea[i] for i, u in enumerate(rho)}, {u: gy[i] for i, u in enumerate(rho)}
    s, v, w, r = rand_scalars(rng, n14), rand_scalars(rng, n14, 7), rand_scalars(rng, n14, 7), rand_scalars(rng, n14, 16)
    table = lw11.encrypt_table(bn254, g2y)
    res = alternate({"encrypt_batch (table built once)": lambda: lw11.encrypt_batch(bn254, e_alpha, egg, g2y, m, rho, msgs, s, v, w, r, table=table)}, args.reps)
    table.close()
    doc["planners"]["lw11_encrypt_16_rows"] = {"ciphertexts": n14, "rows": 16, "cols": 8, **res}
    save()
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
