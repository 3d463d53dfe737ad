"""AFP25 KeyGen / Encrypt / ComputeKey and Waters11 SetUp (gopairingbasedcryptography_amd/afp25.py, waters11.py) on HBM-resident data, route
against route to the same bytes, with the timing helpers of tools/scalar_mul_rows_bench.py.  At 2^log_n items:

  * encrypt_batch under one label: plain, tables=, and tables= + gt_table=, and the stages on their own — C1 by the reference's operations
    against C1 from the three indexed sums, and the three forms of C2 (gt_exp, gt_table, "items"); the three-leg comparison runs twice, and
    the difference between the two runs is the run-to-run spread the others are read against;
  * route "labels" (label_bases included) against route "items" with the labels drawn from L = 1, 16, 2^10, n / 8, n / 4, n / 2 and all distinct; `crossover` holds
    the neighbouring measured shares between which the winner changes (`winner_changes_between`: the result to read) and, beside it, where
    the two would meet on a straight line through the labels route's measurements, which need not fit them;
  * keygen at B = 256 and 1024 against the expression gwww25.keygen uses — Python pow, one upload — as the comparison side;
  * compute_key_batch at 2^10 batches;
  * BASELINE config 5 from keys to messages, B = 256 x 2^(log_n - 8) batches, as ONE timed pass per repetition — keygen, srs_table,
    encrypt_tables, label_points, label_bases, encrypt_batch, digests_ragged, compute_key_batch, decrypt_batches_ragged, every message
    compared on the device — with C2 by gt_exp against C2 from a GTFixedBase over the 256 label bases built inside the pass; the same
    passes with the two per-key tables built beforehand, those builds alone, and every stage alone;
  * waters11.setup over a universe of 2^10 attributes.
Seeded inputs; the legs of a comparison alternate inside one repetition loop; the output bytes of the legs are compared before any time is
reported; device events around calls that end in their own waits.  One process, one device, device tensors only: it fails without a GPU.
Writes one JSON document (profiles/afp25_scheme.json records a run), rewritten after every section.

    python tools/afp25_scheme_bench.py [--reps 5] [--log-n 16] [--out profiles/afp25_scheme.json]"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopairingbasedcryptography_amd import _lib, _plan, afp25, bn254, waters11  # noqa: E402
from gopairingbasedcryptography_amd._buffers import R_ORDER  # noqa: E402
from scalar_mul_rows_bench import alternate, dev, rand_scalars  # noqa: E402


def same(a, b):
    return all(bool(torch.equal(x, y)) for x, y in zip(a, b))


def scalars(rng, n):
    """n canonical scalar rows on the device"""
    k = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    k[:, 31] &= 0x1F
    return dev(k)


def messages(n, rng):
    g1, g2 = bn254.generators()
    e = dev(np.asarray(bn254.pair_batch(g1, g2)).reshape(1, 384))
    return bn254.gt_exp(e.expand(n, 384).contiguous().reshape(-1), rand_scalars(rng, n).reshape(-1)).reshape(n, 384)


def labels(L, rng):
    """L distinct 16-byte labels as one device buffer with its offsets"""
    data = np.zeros((L, 16), dtype=np.uint8)
    data[:, :8] = np.arange(L, dtype="<u8").view(np.uint8).reshape(L, 8)
    data[:, 8:] = rng.integers(0, 256, size=8, dtype=np.uint8)
    return dev(data.reshape(-1)), torch.arange(0, 16 * L + 1, 16, dtype=torch.int64, device="cuda")


def median(res):
    return {leg: s["median_ms"] for leg, s in res.items()}


def encrypt_section(n, reps, rng):
    mpk = afp25.keygen(bn254, 4, scalars(rng, 1), scalars(rng, 1))
    msgs, ids, r1, r2 = messages(n, rng), scalars(rng, n), scalars(rng, n), scalars(rng, n)
    points = afp25.label_points(bn254, *labels(1, rng))
    bases = afp25.label_bases(bn254, mpk, points)
    tables, gt_table = afp25.encrypt_tables(bn254, mpk), bn254.GTFixedBase(bases)
    out = {}
    run = lambda name, **kw: lambda: out.__setitem__(name, afp25.encrypt_batch(bn254, mpk, msgs, ids, r1, r2, points, bases=bases, **kw))
    legs = {"plain": run("plain"), "tables": run("tables", tables=tables), "tables_gt_table": run("both", tables=tables, gt_table=gt_table)}
    for fn in legs.values():
        fn()
    items = afp25.encrypt_batch(bn254, mpk, msgs, ids, r1, r2, points, tables=tables, route="items")
    torch.cuda.synchronize()
    equal = same(out["plain"], out["tables"]) and same(out["plain"], out["both"]) and same(out["plain"], items)
    res, again = alternate(legs, reps), alternate(legs, reps)
    out.clear()
    g2 = dev(np.asarray(bn254.generators()[1]))
    pub = {k: dev(np.asarray(mpk[k])) for k in ("G2ExpTau", "G2ExpMsk")}
    neg = dev(bn254.g2_neg(bn254.generators()[1]))
    flat = lambda x: x.reshape(-1)
    row = lambda *index: _plan.index_rows(np.array([index]), msgs)

    def c1_plain():
        a01 = bn254.g2_sub(bn254.g2_scalar_mul_base(flat(ids)), pub["G2ExpTau"])
        bn254.g2_add(bn254.g2_scalar_mul(g2, flat(r1)), bn254.g2_scalar_mul(pub["G2ExpMsk"], flat(r2)))
        bn254.g2_scalar_mul(flat(a01), flat(r1))
        bn254.g2_scalar_mul(neg, flat(r2))

    def c1_tables():
        r1id, nr1, nr2 = bn254.fr_mul(flat(r1), flat(ids)), bn254.fr_neg(flat(r1)), bn254.fr_neg(flat(r2))
        tables.indexed(row(0, 1), afp25._pairs_of(r1, r2, n), terms=2)
        tables.indexed(row(0, 2), afp25._pairs_of(r1id, nr1, n), terms=2)
        tables.indexed(row(0), flat(nr2), terms=1)

    def c2_items():
        P = bn254.g1_scalar_mul(flat(points), bn254.fr_neg(flat(r2)))
        bn254.gt_mul(flat(bn254.multi_pair_fixed_q(flat(P), pub["G2ExpMsk"])), flat(msgs))
    stages = alternate({"c1_plain": c1_plain, "c1_tables": c1_tables,
                        "c2_gt_exp": lambda: bn254.gt_mul(flat(bn254.gt_exp(flat(bases.expand(n, 384).contiguous()), flat(r2))), flat(msgs)),
                        "c2_gt_table": lambda: bn254.gt_mul(flat(gt_table.indexed(row(0), flat(r2), terms=1)[0]), flat(msgs)),
                        "c2_items": c2_items, "gt_table_build_and_close": lambda: bn254.GTFixedBase(bases).close(),
                        "encrypt_tables_build_and_close": lambda: afp25.encrypt_tables(bn254, mpk).close()}, reps)
    tables.close(), gt_table.close()
    torch.cuda.empty_cache()
    spread = max(abs(res[leg]["median_ms"] - again[leg]["median_ms"]) / res[leg]["median_ms"] for leg in legs)
    return {"items": n, "labels": 1, "same_bytes": equal, **res, "second_run": again, "spread_between_runs": spread, "stages": stages,
            "speedup_tables_over_plain": res["plain"]["median_ms"] / res["tables"]["median_ms"],
            "speedup_tables_gt_table_over_plain": res["plain"]["median_ms"] / res["tables_gt_table"]["median_ms"],
            "items_per_s_tables_gt_table": n / res["tables_gt_table"]["median_ms"] * 1e3}


def routes_section(n, reps, rng):
    mpk = afp25.keygen(bn254, 4, scalars(rng, 1), scalars(rng, 1))
    msgs, ids, r1, r2 = messages(n, rng), scalars(rng, n), scalars(rng, n), scalars(rng, n)
    tables = afp25.encrypt_tables(bn254, mpk)
    doc = {"items": n, "routes": []}
    for L in (1, 16, 1 << 10, n // 8, n // 4, n // 2, n):
        points = afp25.label_points(bn254, *labels(L, rng))
        label_of = np.concatenate([np.arange(L), rng.integers(0, L, size=n - L)])[rng.permutation(n)] if L > 1 else None
        out = {}
        run = lambda route: lambda: out.__setitem__(route, afp25.encrypt_batch(bn254, mpk, msgs, ids, r1, r2, points, label_of, tables=tables, route=route))
        legs = {"labels": run("labels"), "items": run("items")}
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        equal = same(out["labels"], out["items"])
        res = alternate(legs, reps)
        out.clear()
        torch.cuda.empty_cache()
        doc["routes"].append({"labels": L, "distinct_over_total": L / n, "same_bytes": equal, **res, "winner": min(legs, key=lambda leg: res[leg]["median_ms"])})
    tables.close()
    x = [r["distinct_over_total"] for r in doc["routes"]]
    slope, offset = np.polyfit(x, [r["labels"]["median_ms"] for r in doc["routes"]], 1)
    items = float(np.median([r["items"]["median_ms"] for r in doc["routes"]]))
    flips = [(p["distinct_over_total"], q["distinct_over_total"]) for p, q in zip(doc["routes"], doc["routes"][1:]) if p["winner"] != q["winner"]]
    doc["crossover"] = {"labels_ms_at_0": float(offset), "labels_ms_per_unit_share": float(slope), "items_ms": items,
                        "distinct_over_total": float((items - offset) / slope) if slope > 0 else None,
                        "winner_changes_between": flips, "default_route": "labels"}
    return doc


def keygen_section(reps, rng):
    out = []
    for B in (256, 1024):
        tau, msk = scalars(rng, 1), scalars(rng, 1)
        tau_int, msk_int = (int.from_bytes(x.cpu().numpy().tobytes(), "little") for x in (tau, msk))
        got = {}

        def host_pow():
            """the expression gwww25.keygen uses for its powers: Python pow, one upload, the same two generator calls and the download"""
            rows = dev(_plan.scalar_rows([pow(tau_int, i, R_ORDER) for i in range(1, B + 1)]))
            in_g1 = bn254.g1_scalar_mul_base(rows.reshape(-1))
            in_g2 = bn254.g2_scalar_mul_base(dev(_plan.scalar_rows([tau_int, msk_int])).reshape(-1))
            got["host"] = (in_g1.cpu().numpy(), in_g2.cpu().numpy())
        legs = {"device_chain": lambda: got.__setitem__("device", afp25.keygen(bn254, B, tau, msk)), "host_pow": host_pow}
        res = alternate(legs, reps)
        equal = got["device"]["G1ExpTauPowers"].tobytes() == got["host"][0].tobytes() and got["device"]["G2ExpTau"].tobytes() == got["host"][1][0].tobytes()
        powers = alternate({"tau_powers": lambda: afp25.tau_powers(bn254, tau, B)}, reps)
        out.append({"B": B, "same_bytes": equal, **res, **powers, "faster": min(legs, key=lambda leg: res[leg]["median_ms"])})
    return out


def compute_key_section(k, reps, rng):
    msk = scalars(rng, 1)
    D = bn254.g1_scalar_mul_base(scalars(rng, k).reshape(-1)).reshape(k, 64)
    lab = labels(k, rng)
    points = afp25.label_points(bn254, *lab)
    res = alternate({"compute_key_batch": lambda: afp25.compute_key_batch(bn254, msk, D, points), "label_points": lambda: afp25.label_points(bn254, *lab)}, reps)
    return {"batches": k, **res}


def round_trip_section(n, reps, rng):
    """BASELINE config 5 from keys and messages to messages compared, timed as ONE pass per repetition (device events around the whole
    pass, which ends in the comparison's wait), in two forms of Encrypt that alternate: C2 by gt_exp on the gathered label bases, and C2
    from a GTFixedBase over the k label bases BUILT INSIDE the pass — a label belongs to its batch, so that table serves B powers per base
    and is a per-batch cost.  The per-key tables (srs_table, encrypt_tables) are built inside the pass as well; `per_key_builds` times them
    alone, and `pass_tables_prebuilt` is the pass without them.  The stage medians are each stage timed alone on the gt_exp form."""
    B = 256
    k = n // B
    tau, msk = scalars(rng, 1), scalars(rng, 1)
    msgs, ids, r1, r2 = messages(n, rng), scalars(rng, n), scalars(rng, n), scalars(rng, n)
    counts, label_of, lab = [B] * k, np.repeat(np.arange(k), B), labels(k, rng)
    g1 = bn254.generators()[0]
    verdict = {}

    def encrypt(mpk, tables, points, form):
        if form == "gt_exp":
            return afp25.encrypt_batch(bn254, mpk, msgs, ids, r1, r2, points, label_of, tables=tables)            # label_bases inside
        gt_table = bn254.GTFixedBase(afp25.label_bases(bn254, mpk, points))
        try:
            return afp25.encrypt_batch(bn254, mpk, msgs, ids, r1, r2, points, label_of, tables=tables, gt_table=gt_table)
        finally:
            gt_table.close()

    def whole(form, prebuilt=None):
        def run():
            mpk = afp25.keygen(bn254, B, tau, msk)
            table, tables = prebuilt or (afp25.srs_table(bn254, g1, mpk["G1ExpTauPowers"]), afp25.encrypt_tables(bn254, mpk))
            try:
                points = afp25.label_points(bn254, *lab)
                C1, C2 = encrypt(mpk, tables, points, form)
                D = afp25.digests_ragged(bn254, table, ids, counts)
                sk = afp25.compute_key_batch(bn254, msk, D, points)
                m, ok = afp25.decrypt_batches_ragged(bn254, table, ids, counts, sk, C1, C2, D)
                verdict[form] = verdict.get(form, True) and bool(torch.equal(m, msgs)) and bool(ok.all())      # the pass's one wait
            finally:
                if prebuilt is None:
                    table.close(), tables.close()
        return run
    passes = alternate({"pass_gt_exp": whole("gt_exp"), "pass_gt_table_built_inside": whole("gt_table")}, reps)
    mpk = afp25.keygen(bn254, B, tau, msk)
    builds = alternate({"srs_table": lambda: afp25.srs_table(bn254, g1, mpk["G1ExpTauPowers"]).close(),
                        "encrypt_tables": lambda: afp25.encrypt_tables(bn254, mpk).close()}, reps)
    kept = afp25.srs_table(bn254, g1, mpk["G1ExpTauPowers"]), afp25.encrypt_tables(bn254, mpk)
    table, tables = kept
    prebuilt = alternate({"pass_gt_exp": whole("gt_exp", kept), "pass_gt_table_built_inside": whole("gt_table", kept)}, reps)
    points = afp25.label_points(bn254, *lab)
    bases = afp25.label_bases(bn254, mpk, points)
    s = {}
    enc = alternate({"encrypt_gt_exp": lambda: s.__setitem__("ct", encrypt(mpk, tables, points, "gt_exp")),
                     "encrypt_gt_table_built_inside": lambda: s.__setitem__("ct2", encrypt(mpk, tables, points, "gt_table")),
                     "gt_table_build_and_close": lambda: bn254.GTFixedBase(bases).close()}, reps)
    equal = same(s["ct"], s["ct2"])
    dig = lambda: s.__setitem__("D", afp25.digests_ragged(bn254, table, ids, counts))
    dig()
    key = lambda: s.__setitem__("sk", afp25.compute_key_batch(bn254, msk, s["D"], points))
    key()
    dec = lambda: s.__setitem__("m", afp25.decrypt_batches_ragged(bn254, table, ids, counts, s["sk"], s["ct"][0], s["ct"][1], s["D"]))
    stages = dict(enc)
    for name, fn in (("keygen", lambda: afp25.keygen(bn254, B, tau, msk)), ("label_points", lambda: afp25.label_points(bn254, *lab)),
                     ("label_bases", lambda: afp25.label_bases(bn254, mpk, points)), ("digests_ragged", dig), ("compute_key_batch", key),
                     ("decrypt_batches_ragged", dec)):
        stages.update(alternate({name: fn}, reps))
    table.close(), tables.close()
    torch.cuda.empty_cache()
    best = min(passes, key=lambda leg: passes[leg]["median_ms"])
    return {"B": B, "batches": k, "items": n, "every_message_recovered": all(verdict.values()) and len(verdict) == 2, "encrypt_forms_same_bytes": equal,
            "passes_with_per_key_builds": passes, "passes_tables_prebuilt": prebuilt, "per_key_builds": builds, "stage_medians_each_timed_alone": stages,
            "faster_pass": best, "items_per_s_with_per_key_builds": n / passes[best]["median_ms"] * 1e3,
            "items_per_s_tables_prebuilt": n / min(v["median_ms"] for v in prebuilt.values()) * 1e3}


def waters11_section(U, reps, rng):
    alpha, a, tau = scalars(rng, 1), scalars(rng, 1), scalars(rng, U)
    universe = waters11.universe_range(100, 100 + U)
    g1, g2 = bn254.generators()
    gt_table = bn254.GTFixedBase(np.asarray(bn254.pair_batch(g1, g2)).reshape(1, 384))
    got = {}
    legs = {"setup": lambda: got.__setitem__("plain", waters11.setup(bn254, universe, alpha, a, tau)),
            "setup_gt_table": lambda: got.__setitem__("table", waters11.setup(bn254, universe, alpha, a, tau, gt_table=gt_table))}
    res = alternate(legs, reps)
    gt_table.close()
    equal = got["plain"][0]["e_alpha"].tobytes() == got["table"][0]["e_alpha"].tobytes() and all(got["plain"][0]["h"][u].tobytes() == got["table"][0]["h"][u].tobytes() for u in universe)
    return {"universe": U, "same_bytes": equal, **res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "afp25_scheme.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/afp25_scheme_bench.py needs a GPU")
    bn254.init(0)
    rng = np.random.default_rng(2025)
    n = 1 << args.log_n
    doc = {"tool": "tools/afp25_scheme_bench.py", "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
           "library": os.path.relpath(_lib.LIB_PATH, ROOT), "reps": args.reps, "log_n": args.log_n, "encrypt": "not measured", "routes": "not measured",
           "keygen": "not measured", "compute_key": "not measured", "round_trip": "not measured", "waters11_setup": "not measured",
           "unmeasured": "host arrays in (staging included) and more than one device"}

    def save():
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    for name, fn in (("encrypt", lambda: encrypt_section(n, args.reps, rng)), ("routes", lambda: routes_section(n, args.reps, rng)),
                     ("keygen", lambda: keygen_section(args.reps, rng)), ("compute_key", lambda: compute_key_section(1 << 10, args.reps, rng)),
                     ("round_trip", lambda: round_trip_section(n, args.reps, rng)), ("waters11_setup", lambda: waters11_section(1 << 10, args.reps, rng))):
        doc[name] = fn()
        save()
        print(name, "done", flush=True)
    e, rt = doc["encrypt"], doc["round_trip"]
    print(json.dumps({"encrypt": {"same_bytes": e["same_bytes"], **median({k: e[k] for k in ("plain", "tables", "tables_gt_table")}), "spread": e["spread_between_runs"],
                                  "stages": median(e["stages"])},
                      "routes": [{"labels": r["labels"], "same_bytes": r["same_bytes"], **median({k: r[k] for k in ("labels", "items")})} for r in doc["routes"]["routes"]],
                      "crossover": doc["routes"]["crossover"],
                      "keygen": [{"B": r["B"], "same_bytes": r["same_bytes"], **median({k: r[k] for k in ("device_chain", "host_pow", "tau_powers")})} for r in doc["keygen"]],
                      "compute_key": median({k: v for k, v in doc["compute_key"].items() if isinstance(v, dict)}),
                      "round_trip": {"every_message_recovered": rt["every_message_recovered"], "with_per_key_builds": median(rt["passes_with_per_key_builds"]),
                                     "tables_prebuilt": median(rt["passes_tables_prebuilt"]), "per_key_builds": median(rt["per_key_builds"]),
                                     "stages_alone": median(rt["stage_medians_each_timed_alone"])},
                      "waters11_setup": {"same_bytes": doc["waters11_setup"]["same_bytes"], **median({k: doc["waters11_setup"][k] for k in ("setup", "setup_gt_table")})}}))


if __name__ == "__main__":
    main()
