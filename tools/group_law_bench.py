"""2^20 HBM-resident G1 / G2 additions, subtractions and doublings (k_g1_add .. k_g2_dbl) against the variable-base scalar
multiplication of the same points (gpbc_g1/g2_scalar_mul_batch_dev, one base per scalar), alternated repetition by repetition
after a warm-up and timed with HIP events on the current stream; medians.  Also the host-pointer rates (PCIe-bound) and the
broadcast form (one b for all).  Writes one JSON document (profiles/group_law_2_20.json records a run).

    python tools/group_law_bench.py [--n 1048576] [--reps 5] [--out FILE]

GPBC_LIB_PATH selects another build of the library (a GROUP_K variant, for instance)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopairingbasedcryptography_amd import _lib, bn254  # noqa: E402

HBM_PEAK_TBS = 8.0                       # MI355X HBM3E peak, TB/s


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.n
    bn254.init(0)
    lib = _lib.load()
    rng = np.random.default_rng(20)
    doc = {"n": n, "reps": args.reps, "lib": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0),
           "hbm_peak_TBs": HBM_PEAK_TBS, "groups": {}}
    for name, width, smul in (("g1", 64, bn254.g1_scalar_mul), ("g2", 128, bn254.g2_scalar_mul)):
        gen = torch.from_numpy(bn254.generators()[1 if name == "g2" else 0].copy()).cuda()
        k = rng.integers(0, 256, size=(3, n, 32), dtype=np.uint8)
        k[:, :, 31] &= 0x1F
        ks = [torch.from_numpy(k[i].reshape(-1).copy()).cuda() for i in range(3)]
        A, B = smul(gen, ks[0]), smul(gen, ks[1])                       # random points (fixed-base path: one base)
        out = torch.empty_like(A)
        sm_out = torch.empty_like(A)
        add, sub, dbl = (getattr(bn254, "%s_%s" % (name, op)) for op in ("add", "sub", "double"))
        ops = {"add": lambda: add(A, B, out=out), "sub": lambda: sub(A, B, out=out), "dbl": lambda: dbl(A, out=out),
               "add_broadcast": lambda: add(A, B[:1], out=out)}
        scalar_mul = lambda: smul(A, ks[2], out=sm_out)                 # one base per scalar: the variable-base kernel
        for f in list(ops.values()) + [scalar_mul]:                      # warm-up (and the workspaces' first growth)
            f()
        torch.cuda.synchronize()
        t = {key: [] for key in list(ops) + ["scalar_mul"]}
        for _ in range(args.reps):
            for key, f in ops.items():
                t[key].append(timed(f))
                t["scalar_mul"].append(timed(scalar_mul))
        med = {key: statistics.median(v) for key, v in t.items()}
        g = {"ms": med, "ms_all": t, "scalar_mul_ms": med["scalar_mul"]}
        for key in ops:
            moved = (3 if key in ("add", "sub") else 2) * n * width         # read a (and b), write out
            if key == "add_broadcast":
                moved = 2 * n * width
            g[key] = {"ms": med[key], "ratio_to_scalar_mul": med[key] / med["scalar_mul"], "bytes": moved,
                      "GBs": moved / med[key] / 1e6, "hbm_peak_share": moved / med[key] / 1e9 / HBM_PEAK_TBS,
                      "Mops": n / med[key] / 1e3}
        # host-pointer entries (sharding off the table: one device), for the record
        An, Bn = A.cpu().numpy(), B.cpu().numpy()
        On = np.empty_like(An)
        host = {}
        for key, f in (("add", lambda: add(An, Bn, out=On)), ("sub", lambda: sub(An, Bn, out=On)), ("dbl", lambda: dbl(An, out=On)),
                       ("add_broadcast", lambda: add(An, Bn[:1], out=On))):
            f()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                f()
                ts.append((time.perf_counter() - t0) * 1e3)
            host[key] = {"ms": statistics.median(ts), "Mops": n / statistics.median(ts) / 1e3}
        g["host"] = host
        doc["groups"][name] = g
        print(name, " ".join("%s %.3f ms (1/%.0f of scalar mul %.2f ms)" % (key, med[key], med["scalar_mul"] / med[key], med["scalar_mul"]) for key in ops), flush=True)
        print(name, "host", " ".join("%s %.2f ms" % (key, v["ms"]) for key, v in host.items()), flush=True)
        del A, B, out, sm_out, ks
        lib.gpbc_release_workspaces()
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
