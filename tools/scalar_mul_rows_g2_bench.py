"""The G2 row tables (one base per row of m scalars: csrc/rows29_g2.hip.hpp, csrc/gpbc_rows_g2.hip) on HBM-resident data, route against
route to the same bytes, and the planner built on them — the G2 sibling of tools/scalar_mul_rows_bench.py, whose timing helpers it uses:

  * G2 at 2^20 outputs for m in {4, 8, 16, 32, 64, 256, 4096}: the row tables (GPBC_ROWS_G2_TABLE_MIN=2 in the environment takes them at
    every row length they serve), the table-free row kernel (GPBC_ROWS_G2_TABLE_MIN=0 never takes them) and g2_scalar_mul with one base
    per scalar on the bases expanded by repeat_interleave, the expansion included;
  * the m = 16 comparison a second time: the difference between the two runs is the run-to-run spread the others are read against;
  * bsw07.keygen_batch at 2^12 users x 32 attributes and 2^14 x 16, H2 given as rows, tables forced against table-free forced.  At
    2^14 users a row has 16 384 scalars: the entry sends such rows through the transient 8-bit table whatever the override says, and
    both legs take that route.
Seeded inputs; the legs of a comparison alternate inside one repetition loop; the output bytes of the legs are compared before any time
is reported; device events.  One process, one device.  Writes one JSON document (profiles/shared_base_rows_g2.json records a run),
rewritten after every section.  `verdict` gives the crossover: the smallest measured m from which the tables beat the table-free route at
that m and at every larger measured m by more than the spread (null: none), beside ROWS_G2_TABLE_MIN as built.

    python tools/scalar_mul_rows_g2_bench.py [--reps 6] [--log-n 20] [--out FILE]"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopairingbasedcryptography_amd import _lib, bn254, bsw07  # noqa: E402
from scalar_mul_rows_bench import ROW_LENGTHS, alternate, points, rand_scalars  # noqa: E402

KNOB = "GPBC_ROWS_G2_TABLE_MIN"
LEGS = ("table", "table_free", "expanded")


def with_knob(value, fn):
    """fn under GPBC_ROWS_G2_TABLE_MIN=value; the library reads it at every call"""
    def run():
        old = os.environ.get(KNOB)
        os.environ[KNOB] = value
        try:
            return fn()
        finally:
            if old is None:
                os.environ.pop(KNOB, None)
            else:
                os.environ[KNOB] = old
    return run


def dispatched(m):
    """the route the library as built takes for a G2 row length"""
    if m >= bn254.ROWS_TABLE_MAX:
        return "transient_8bit_table"
    return "table" if m >= bn254.ROWS_G2_TABLE_MIN else "table_free"


def rows_section(m, n, reps, rng):
    nbase = n // m
    bases = points(True, nbase, "rows-g2-%d" % m)
    k = rand_scalars(rng, nbase * m).reshape(-1)
    flat = bases.reshape(-1)
    out = {}
    legs = {"table": with_knob("2", lambda: out.__setitem__("table", bn254.g2_scalar_mul(flat, k))),
            "table_free": with_knob("0", lambda: out.__setitem__("table_free", bn254.g2_scalar_mul(flat, k))),
            "expanded": lambda: out.__setitem__("expanded", bn254.g2_scalar_mul(bases.repeat_interleave(m, dim=0).reshape(-1), k))}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(out[name].reshape(-1), out["expanded"].reshape(-1))) for name in legs)
    res = alternate(legs, reps)
    del out
    torch.cuda.empty_cache()
    doc = {"group": "G2", "m": m, "nbase": nbase, "outputs": nbase * m, "same_bytes": same, "dispatch": dispatched(m), **res,
           **{name + "_Mmul_per_s": nbase * m / res[name]["median_ms"] / 1e3 for name in legs}}
    doc["speedup_table_over_table_free"] = res["table_free"]["median_ms"] / res["table"]["median_ms"]
    doc["speedup_table_over_expanded"] = res["expanded"]["median_ms"] / res["table"]["median_ms"]
    doc["winner"] = min(LEGS, key=lambda leg: res[leg]["median_ms"])
    return doc


def keygen_section(users, attrs, reps, rng):
    h2 = points(True, attrs, "keygen-g2-%d" % attrs)
    _, msk = bsw07.setup(bn254, rand_scalars(rng, 1), rand_scalars(rng, 1))
    r, rj = rand_scalars(rng, users), rand_scalars(rng, users, attrs)
    out = {}
    run = lambda name: lambda: out.__setitem__(name, bsw07.keygen_batch(bn254, msk, h2, r, rj))
    legs = {"table": with_knob("2", run("table")), "table_free": with_knob("0", run("table_free"))}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(a, b)) for a, b in zip(out["table"], out["table_free"]))
    res = alternate(legs, reps)
    del out
    torch.cuda.empty_cache()
    route = dispatched(users)
    return {"users": users, "attributes": attrs, "row_length": users, "same_bytes": same, "dispatch": route, **res,
            "speedup_table_over_table_free": res["table_free"]["median_ms"] / res["table"]["median_ms"],
            "winner": "transient_8bit_table (both legs)" if route == "transient_8bit_table" else min(legs, key=lambda leg: res[leg]["median_ms"]),
            "note": "H2 given as rows: hashing is not timed; the whole planner is: D, dj_prime, the row call, the additions"}


def verdict(doc):
    by_m = {s["m"]: s for s in doc["g2_rows"]}
    again = doc["g2_rows_m16_again"]
    spread = max(abs(again[leg]["median_ms"] / by_m[16][leg]["median_ms"] - 1.0) for leg in LEGS) if 16 in by_m and again else None
    ms = sorted(by_m)
    margin = spread or 0.0
    wins = [m for m in ms if by_m[m]["table"]["median_ms"] * (1.0 + margin) < by_m[m]["table_free"]["median_ms"]]
    from_m = next((m for m in ms if all(x in wins for x in ms if x >= m)), None)
    return {"run_to_run_spread": spread, "tables_beat_table_free_from_m": from_m, "ROWS_G2_TABLE_MIN_as_built": bn254.ROWS_G2_TABLE_MIN,
            "winner_by_m": {str(m): by_m[m]["winner"] for m in ms}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bn254.init(0)
    rng = np.random.default_rng(2007)
    n = 1 << args.log_n
    doc = {"tool": "tools/scalar_mul_rows_g2_bench.py", "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
           "library": os.path.relpath(_lib.LIB_PATH, ROOT), "reps": args.reps, "log_n": args.log_n, "g2_rows": [], "g2_rows_m16_again": None, "keygen": [],
           "verdict": None, "unmeasured": "the host-pointer entries (staging included) and more than one device"}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
    for m in ROW_LENGTHS:
        if m <= n:
            doc["g2_rows"].append(rows_section(m, n, args.reps, rng))
            save()
    if 16 <= n:
        doc["g2_rows_m16_again"] = rows_section(16, n, args.reps, rng)
        doc["verdict"] = verdict(doc)
        save()
    for users, attrs in ((1 << max(args.log_n - 8, 0), 32), (1 << max(args.log_n - 6, 0), 16)):
        doc["keygen"].append(keygen_section(users, attrs, args.reps, rng))
        save()
    print(json.dumps({"verdict": doc["verdict"], "g2": {s["m"]: {leg: s[leg]["median_ms"] for leg in LEGS} for s in doc["g2_rows"]},
                      "keygen": [{k: (s[k]["median_ms"] if isinstance(s[k], dict) else s[k]) for k in ("users", "attributes", "table", "table_free", "winner")} for s in doc["keygen"]]}))


if __name__ == "__main__":
    main()
