"""SW05 Encrypt of both universes and the d + 1 pair Decrypt (gopairingbasedcryptography_amd/sw05.py) on HBM-resident data, route
against route to the same bytes, with the timing helpers of tools/scalar_mul_rows_bench.py.  At 2^log_n ciphertexts x `attrs` attributes:

  * Universe.lookup alone over range and values universes of 64 and 4096 attributes;
  * encrypt_batch over a values universe of 64 (and of 1024) with and without table= / gt_table=, and its stages on their own: the
    lookup, the blinding factor, and the G2 stage as a gather + g2_scalar_mul against FixedBase.indexed;
  * encrypt_batch_large at n = 32, routes "dedupe" and "fold", with the attribute values drawn from 64, from 4096, with half of them
    distinct and all distinct; `crossover` is where the two routes' times meet on the line through the dedupe route's measurements
    (distinct / total against time) — what sw05.AUTO_DEDUPE_BELOW is set from;
  * decrypt_batch_large_msm against decrypt_batch_large on ciphertexts of encrypt_batch_large whose attributes the key holds, d given.
Seeded inputs; the legs of a comparison alternate inside one repetition loop; the output bytes of the legs are compared before any time
is reported; device events around calls that end in their own waits.  One process, one device.  Writes one JSON document
(profiles/sw05_encrypt.json records a run), rewritten after every section.

    python tools/sw05_encrypt_bench.py [--reps 4] [--log-n 16] [--attrs 24] [--d 16] [--out FILE]"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopairingbasedcryptography_amd import _buffers as bufs, _lib, _plan, bn254, sw05  # noqa: E402
from scalar_mul_rows_bench import alternate, dev, rand_scalars  # noqa: E402

N_LARGE = 32


def same(a, b):
    return all(bool(torch.equal(x, y)) for x, y in zip(a, b))


def small_rows(values):
    """non-negative integers below 2^63 as scalar rows [.., 32] on the device"""
    v = np.ascontiguousarray(np.asarray(values, dtype="<u8"))
    out = np.zeros(v.shape + (32,), dtype=np.uint8)
    out[..., :8] = v.view(np.uint8).reshape(v.shape + (8,))
    return dev(out)


def universes(size, rng):
    """(range universe 100 .. 100 + size, values universe of `size` full-size values, their members as rows [size, 32] each)"""
    values = rng.integers(0, 256, size=(size, 32), dtype=np.uint8)
    values[:, 31] &= 0x1F                                                     # below r: the rows are the canonical values
    return (sw05.Universe.range(100, 100 + size), sw05.Universe.from_values(values)), (small_rows(np.arange(100, 100 + size)), dev(values))


def messages(n, rng):
    g1, g2 = bn254.generators()
    e = dev(np.asarray(bn254.pair_batch(g1, g2)).reshape(1, 384))
    return bn254.gt_exp(e.expand(n, 384).contiguous().reshape(-1), rand_scalars(rng, n).reshape(-1)).reshape(n, 384)


def lookup_section(n, a, reps, rng):
    out = []
    for size in (64, 4096):
        (u_range, u_values), (m_range, m_values) = universes(size, rng)
        pick = dev(rng.integers(0, size, size=n * a))
        for kind, u, members in (("range", u_range, m_range), ("values", u_values, m_values)):
            attrs = members[pick].reshape(n, a, 32).contiguous()
            index, ok = u.lookup(bn254, attrs)
            right = bool(torch.equal(index.reshape(-1).long(), pick)) and bool(ok.all())
            res = alternate({"lookup": lambda: u.lookup(bn254, attrs)}, reps)
            out.append({"universe": kind, "size": size, "rows": n * a, "positions_right": right, **res,
                        "ns_per_attribute": res["lookup"]["median_ms"] * 1e6 / (n * a)})
    return out


def encrypt_section(size, n, a, reps, rng):
    (_, u), (_, members) = universes(size, rng)
    pp, _ = sw05.setup(bn254, u, rand_scalars(rng, 1), rand_scalars(rng, size))
    attrs = members[dev(rng.integers(0, size, size=n * a))].reshape(n, a, 32).contiguous()
    msgs, s = messages(n, rng), rand_scalars(rng, n)
    build = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    build[0].record()
    table = sw05.encrypt_table(bn254, pp)
    build[1].record()
    build[1].synchronize()
    gt_table = bn254.GTFixedBase(pp["Y"].reshape(1, 384))
    out = {}
    run = lambda name, **kw: lambda: out.__setitem__(name, sw05.encrypt_batch(bn254, u, pp, attrs, msgs, s, **kw))
    legs = {"plain": run("plain"), "table": run("table", table=table), "table_gt_table": run("both", table=table, gt_table=gt_table)}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    equal = same(out["plain"], out["table"]) and same(out["plain"], out["both"]) and bool(out["plain"][2].all())
    res = alternate(legs, reps)
    out.clear()
    index, _ = u.lookup(bn254, attrs)
    sa = s.reshape(n, 1, 32).expand(n, a, 32).contiguous().reshape(-1)
    flat_index = index.reshape(n * a, 1).contiguous()
    stages = alternate({"lookup": lambda: u.lookup(bn254, attrs),
                        "blind_gt_exp": lambda: _plan.blind(bn254, pp["Y"], s.reshape(-1), msgs, n),
                        "blind_gt_table": lambda: sw05._blind(bn254, pp["Y"], s.reshape(-1), msgs, n, gt_table),
                        "g2_gather_scalar_mul": lambda: bn254.g2_scalar_mul(bufs.flat(bufs.take(pp["T"], index.reshape(-1))), sa),
                        "g2_indexed": lambda: table.indexed(flat_index, sa, terms=1)}, reps)
    table.close(), gt_table.close()
    torch.cuda.empty_cache()
    g2 = lambda name: n * a / stages[name]["median_ms"] / 1e3
    return {"universe": "values", "size": size, "ciphertexts": n, "attributes": a, "same_bytes": equal, **res, "stages": stages,
            "table_build_ms": build[0].elapsed_time(build[1]), "table_MiB": size * 2,
            "g2_gather_scalar_mul_Mmul_per_s": g2("g2_gather_scalar_mul"), "g2_indexed_Mmul_per_s": g2("g2_indexed"),
            "speedup_table_over_plain": res["plain"]["median_ms"] / res["table"]["median_ms"]}


def large_section(n, a, d, reps, rng):
    pp, msk = sw05.setup_large(bn254, N_LARGE, rand_scalars(rng, 1), rand_scalars(rng, N_LARGE + 1))
    table, nodes = sw05.large_table(bn254, pp)
    msgs, s = messages(n, rng), rand_scalars(rng, n)
    rows = n * a
    pool = rand_scalars(rng, rows)
    pool[:, 31] &= 0x1F
    doc = {"n": N_LARGE, "ciphertexts": n, "attributes": a, "routes": []}
    keep = None
    for label, distinct in (("64", 64), ("4096", 4096), ("half", rows // 2), ("all", rows)):
        if distinct >= rows and label != "all":
            continue
        pick = torch.cat([torch.arange(distinct, device="cuda"), dev(rng.integers(0, distinct, size=rows - distinct))])[dev(rng.permutation(rows))]
        if distinct == 64:                                                    # every ciphertext's attributes distinct: the decrypt section's input
            pick = dev(np.stack([rng.permutation(64)[:a] for _ in range(n)]).reshape(-1))
        attrs = pool[pick].reshape(n, a, 32).contiguous()
        out = {}
        run = lambda route: lambda: out.__setitem__(route, sw05.encrypt_batch_large(bn254, table, N_LARGE, pp, attrs, msgs, s, nodes=nodes, route=route))
        legs = {"dedupe": run("dedupe"), "fold": run("fold")}
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        equal = same(out["dedupe"], out["fold"])
        res = alternate(legs, reps)
        if distinct == 64:
            keep = (attrs, out["dedupe"], pool[:64])
        out = None
        torch.cuda.empty_cache()
        doc["routes"].append({"values_from": label, "distinct_over_total": len(torch.unique(pick)) / rows, "same_bytes": equal, **res,
                              "winner": min(legs, key=lambda leg: res[leg]["median_ms"])})
    x = [r["distinct_over_total"] for r in doc["routes"]]
    slope, offset = np.polyfit(x, [r["dedupe"]["median_ms"] for r in doc["routes"]], 1)
    fold = float(np.median([r["fold"]["median_ms"] for r in doc["routes"]]))
    doc["crossover"] = {"dedupe_ms_at_0": float(offset), "dedupe_ms_per_unit_share": float(slope), "fold_ms": fold,
                        "distinct_over_total": float((fold - offset) / slope) if slope > 0 else None, "AUTO_DEDUPE_BELOW_as_built": sw05.AUTO_DEDUPE_BELOW}
    # Decrypt: one key over the 64 values, every ciphertext shares all its attributes with it
    attrs, (E, e_pp, e_prime), key_attrs = keep
    coeffs, r = rand_scalars(rng, 1, d - 1), rand_scalars(rng, 1, 64)
    dk, Dk = sw05.keygen_batch_large(bn254, table, N_LARGE, msk["y"].cpu().numpy(), coeffs, key_attrs.reshape(1, 64, 32), r)
    key = (key_attrs, dk.reshape(64, 64), Dk.reshape(64, 128))
    out = {}
    legs = {"pairs_2d": lambda: out.__setitem__("2d", sw05.decrypt_batch_large(bn254, key, d, attrs, E, e_pp, e_prime)),
            "pairs_d_plus_1": lambda: out.__setitem__("d1", sw05.decrypt_batch_large_msm(bn254, key, d, attrs, E, e_pp, e_prime))}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    equal = same(out["2d"], out["d1"]) and bool(torch.equal(out["2d"][0], msgs)) and bool(out["2d"][1].all())
    res = alternate(legs, reps)
    table.close()
    doc["decrypt"] = {"d": d, "key_attributes": 64, "messages_recovered_and_equal": equal, **res,
                      "speedup_d_plus_1_over_2d": res["pairs_2d"]["median_ms"] / res["pairs_d_plus_1"]["median_ms"]}
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--attrs", type=int, default=24)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bn254.init(0)
    rng = np.random.default_rng(2005)
    n = 1 << args.log_n
    doc = {"tool": "tools/sw05_encrypt_bench.py", "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
           "library": os.path.relpath(_lib.LIB_PATH, ROOT), "reps": args.reps, "log_n": args.log_n, "attributes": args.attrs, "lookup": None, "encrypt": [],
           "large": None, "unmeasured": "host arrays in (staging included) and more than one device"}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
    doc["lookup"] = lookup_section(n, args.attrs, args.reps, rng)
    save()
    for size in (64, 1024):                                                       # the table of 1024 attributes is 2 GiB
        doc["encrypt"].append(encrypt_section(size, n, args.attrs, args.reps, rng))
        save()
    doc["large"] = large_section(n, args.attrs, args.d, args.reps, rng)
    save()
    med = lambda s, legs: {leg: s[leg]["median_ms"] for leg in legs}
    print(json.dumps({"lookup": [{"universe": s["universe"], "size": s["size"], "ms": s["lookup"]["median_ms"]} for s in doc["lookup"]],
                      "encrypt": [{"size": s["size"], "same_bytes": s["same_bytes"], **med(s, ("plain", "table", "table_gt_table")), "stages": med(s["stages"], s["stages"])} for s in doc["encrypt"]],
                      "large": [{"values_from": r["values_from"], "same_bytes": r["same_bytes"], **med(r, ("dedupe", "fold"))} for r in doc["large"]["routes"]],
                      "crossover": doc["large"]["crossover"], "decrypt": {k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in doc["large"]["decrypt"].items()}}))


if __name__ == "__main__":
    main()
