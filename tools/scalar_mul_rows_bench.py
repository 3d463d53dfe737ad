"""The row form of g1 / g2_scalar_mul (one base per row of m scalars: csrc/rows29.hip.hpp, csrc/gpbc_rows.hip) on HBM-resident data, route
against route to the same bytes, and the planner built on it:

  * G1 at 2^20 outputs for m in {4, 8, 16, 32, 64, 256, 4096}: the row tables (GPBC_ROWS_TABLE_MIN=2 in the environment takes them at
    every row length they serve), the table-free row kernel (GPBC_ROWS_TABLE_MIN=0 never takes them) and the route the engine had before —
    g1_scalar_mul with one base per scalar on the bases expanded by repeat_interleave, the expansion included;
  * the m = 16 comparison a second time: the difference between the two runs is the run-to-run spread the others are read against;
  * G2 at m = 16, the table-free rows against the expanded route (GPBC_ROWS_G2_TABLE_MIN=0 beside the G1 knob: the G2 row tables
    have a tool of their own, tools/scalar_mul_rows_g2_bench.py);
  * lw11.keygen_batch at 2^16 users x 16 attributes and 2^14 x 64, H(GID) given as rows, against the same planner on an engine whose
    g1_scalar_mul expands the rows first.
Seeded inputs; the legs of a comparison alternate inside one repetition loop; the output bytes of the legs are compared before any time
is reported; device events.  One process, one device.  Writes one JSON document (profiles/shared_base_rows.json records a run),
rewritten after every section.  `verdict` says from which measured m on the tables won at every larger one, and whether the library's
dispatch (ROWS_TABLE_MIN as built) ever picks a route that measured slower than the expanded one by more than the spread.

    python tools/scalar_mul_rows_bench.py [--reps 6] [--log-n 20] [--out FILE]"""
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

from gopairingbasedcryptography_amd import _lib, bn254, lw11  # noqa: E402

KNOB = "GPBC_ROWS_TABLE_MIN"
KNOB_G2 = "GPBC_ROWS_G2_TABLE_MIN"           # the G2 tables' own override (csrc/gpbc_rows_g2.hip); this tool's G2 leg is the table-free one
ROW_LENGTHS = (4, 8, 16, 32, 64, 256, 4096)


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
    """every leg warmed up once, then `reps` rounds of all legs in turn, the turn starting one leg later every round (a leg runs in
    the caches and page tables its predecessor leaves: the table leg touches a gigabyte, so no leg always follows it); {name: stats}"""
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in legs}
    names = list(legs)
    for r in range(reps):
        for name in names[r % len(names):] + names[:r % len(names)]:
            ts[name].append(timed(legs[name]))
    return {name: stats(t) for name, t in ts.items()}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rand_scalars(rng, *shape):
    return dev(rng.integers(0, 256, size=shape + (32,), dtype=np.uint8))


def points(g2, n, tag):
    ks = rand_scalars(np.random.default_rng(zlib.crc32(tag.encode())), n)
    return (bn254.g2_scalar_mul_base if g2 else bn254.g1_scalar_mul_base)(ks.reshape(-1)).reshape(n, 128 if g2 else 64)


def with_knob(value, fn):
    """fn under GPBC_ROWS_TABLE_MIN=value and GPBC_ROWS_G2_TABLE_MIN=value (None: as built); the library reads them at every call"""
    def run():
        old = {k: os.environ.get(k) for k in (KNOB, KNOB_G2)}
        for k in old:
            if value is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = value
        try:
            return fn()
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return run


def dispatched(g2, m):
    """the route the library as built takes for a row length"""
    if m >= 16384:
        return "transient_8bit_table"
    return "table" if m >= (bn254.ROWS_G2_TABLE_MIN if g2 else bn254.ROWS_TABLE_MIN) else "table_free"


def rows_section(g2, m, n, reps, rng):
    mul = bn254.g2_scalar_mul if g2 else bn254.g1_scalar_mul
    nbase = n // m
    bases = points(g2, nbase, "rows-%d-%d" % (g2, m))
    k = rand_scalars(rng, nbase * m).reshape(-1)
    flat = bases.reshape(-1)
    out = {}
    legs = {"table_free": with_knob("0", lambda: out.__setitem__("table_free", mul(flat, k))),
            "expanded": lambda: out.__setitem__("expanded", mul(bases.repeat_interleave(m, dim=0).reshape(-1), k))}
    if not g2:
        legs = {"table": with_knob("2", lambda: out.__setitem__("table", mul(flat, k))), **legs}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(out[name].reshape(-1), out["expanded"].reshape(-1))) for name in legs)
    res = alternate(legs, reps)
    del out
    torch.cuda.empty_cache()
    rate = lambda name: nbase * m / res[name]["median_ms"] / 1e3
    doc = {"group": "G2" if g2 else "G1", "m": m, "nbase": nbase, "outputs": nbase * m, "same_bytes": same, "dispatch": dispatched(g2, m), **res,
           **{name + "_Mmul_per_s": rate(name) for name in legs}}
    for name in legs:
        if name != "expanded":
            doc["speedup_%s_over_expanded" % name] = res["expanded"]["median_ms"] / res[name]["median_ms"]
    return doc


class ExpandingEngine:
    """bn254 with the row form of g1_scalar_mul taken away: the rows' bases are expanded first, as a caller had to before"""

    def __getattr__(self, name):
        return getattr(bn254, name)

    @staticmethod
    def g1_scalar_mul(bases, scalars, out=None):
        nbase, n = bases.numel() // 64, scalars.numel() // 32
        if nbase not in (1, n):
            bases = bases.reshape(nbase, 64).repeat_interleave(n // nbase, dim=0).reshape(-1)
        return bn254.g1_scalar_mul(bases, scalars, out)


def keygen_section(users, attrs, reps, rng):
    h = points(False, users, "keygen-%d" % users)
    alpha, y = rand_scalars(rng, attrs), rand_scalars(rng, attrs)
    out = {}
    legs = {"rows": lambda: out.__setitem__("rows", lw11.keygen_batch(bn254, None, alpha, y, h_gid=h)),
            "expanded": lambda: out.__setitem__("expanded", lw11.keygen_batch(ExpandingEngine(), None, alpha, y, h_gid=h))}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(out["rows"], out["expanded"]))
    res = alternate(legs, reps)
    del out
    torch.cuda.empty_cache()
    return {"users": users, "attributes": attrs, "same_bytes": same, "dispatch": dispatched(False, attrs), **res,
            "speedup": res["expanded"]["median_ms"] / res["rows"]["median_ms"], "note": "H(GID) given as rows: hashing is not timed"}


def verdict(doc):
    g1 = {s["m"]: s for s in doc["g1_rows"]}
    again = doc["g1_rows_m16_again"]
    spread = max(abs(again[leg]["median_ms"] / g1[16][leg]["median_ms"] - 1.0) for leg in ("table", "table_free", "expanded")) if 16 in g1 and again else None
    ms = sorted(g1)
    wins = [m for m in ms if g1[m]["table"]["median_ms"] < min(g1[m]["table_free"]["median_ms"], g1[m]["expanded"]["median_ms"])]
    from_m = next((m for m in ms if all(x in wins for x in ms if x >= m)), None)
    slower = []
    for s in doc["g1_rows"] + ([doc["g2_rows_m16"]] if doc["g2_rows_m16"] else []):
        picked = s["dispatch"]
        if picked in s and spread is not None and s[picked]["median_ms"] > s["expanded"]["median_ms"] * (1.0 + spread):
            slower.append({"group": s["group"], "m": s["m"], "route": picked, "ratio_to_expanded": s[picked]["median_ms"] / s["expanded"]["median_ms"]})
    return {"run_to_run_spread": spread, "tables_win_from_m": from_m, "ROWS_TABLE_MIN_as_built": bn254.ROWS_TABLE_MIN,
            "dispatch_slower_than_expanded_beyond_spread": slower}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bn254.init(0)
    rng = np.random.default_rng(2011)
    n = 1 << args.log_n
    doc = {"tool": "tools/scalar_mul_rows_bench.py", "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "library": os.path.relpath(_lib.LIB_PATH, ROOT),
           "reps": args.reps, "log_n": args.log_n, "g1_rows": [], "g1_rows_m16_again": None, "g2_rows_m16": None, "keygen": [], "verdict": None,
           "unmeasured": "the host-pointer entries (staging included) and more than one device"}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
    for m in ROW_LENGTHS:
        if m <= n:
            doc["g1_rows"].append(rows_section(False, m, n, args.reps, rng))
            save()
    if 16 <= n:
        doc["g1_rows_m16_again"] = rows_section(False, 16, n, args.reps, rng)
        doc["g2_rows_m16"] = rows_section(True, 16, n, args.reps, rng)
        doc["verdict"] = verdict(doc)
        save()
    for users, attrs in ((1 << max(args.log_n - 4, 0), 16), (1 << max(args.log_n - 6, 0), 64)):
        doc["keygen"].append(keygen_section(users, attrs, args.reps, rng))
        save()
    print(json.dumps({"verdict": doc["verdict"], "g1": {s["m"]: {leg: s[leg]["median_ms"] for leg in ("table", "table_free", "expanded")} for s in doc["g1_rows"]},
                      "g2_m16": doc["g2_rows_m16"] and {leg: doc["g2_rows_m16"][leg]["median_ms"] for leg in ("table_free", "expanded")},
                      "keygen": [{k: (s[k]["median_ms"] if isinstance(s[k], dict) else s[k]) for k in ("users", "attributes", "rows", "expanded", "speedup")} for s in doc["keygen"]]}))


if __name__ == "__main__":
    main()
