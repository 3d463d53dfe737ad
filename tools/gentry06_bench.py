"""The transcript hash H(u, v, w) and the plain SHA-256 on the device (include/gpbc_bn254_hash.h) on HBM-resident data, and the Gentry06
IBE batches over them:

  (a) k_hash_g1_gt_gt_to_fr alone (gpbc_hash_g1_gt_gt_to_fr_dev), n = 2^16 and 2^20 — kernel time between device events, items/s and the
      bytes it moves (832 read + 32 written per item) over that time;
  (b) the route it replaces, in the same process and alternating with (a) repetition by repetition: gpbc_g1_marshal_batch_dev (compressed)
      and twice gpbc_gt_marshal_batch_dev into device buffers — the DEVICE PART, three launches between device events — then the
      800 B / item copy to pinned host memory, hashlib.sha256 and % r item by item, and the 32 B / item copy back — the WHOLE, a host
      clock around work that ends in a device synchronise.  The two routes' scalars are compared before any time is reported;
  (c) k_sha256 (gpbc_sha256_batch_dev) on 32-byte and on 1 KiB messages, digests and scalars: messages/s and message bytes/s;
  (d) gentry06.keygen_batch / encrypt_batch / decrypt_batch at 2^16 identities for k = 1 and k = 3, device resident, with the time of
      every engine call of one run (device events around each call, summed per entry name).
Every shape is warmed up first, then timed `--reps` times (min / median / max and all samples kept).  One process, one device.  Writes
one JSON document (profiles/gentry06.json records a run).

    python tools/gentry06_bench.py [--reps 5] [--max-log-n 20] [--planner-log-n 16] [--out FILE] [--skip-planner]"""
import argparse
import ctypes
import datetime
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopairingbasedcryptography_amd import _lib, bn254, gentry06  # noqa: E402
from gopairingbasedcryptography_amd._buffers import R_ORDER  # noqa: E402

P = ctypes.c_void_p
HBM_PEAK_BYTES_PER_S = 8.0e12            # MI355X HBM3E, specification; about 6.3e12 is what a plain copy reaches


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return {"min_ms": min(ts), "median_ms": statistics.median(ts), "max_ms": max(ts), "all_ms": ts}


def measure(fn, reps, clock=timed):
    fn()
    torch.cuda.synchronize()
    return stats([clock(fn) for _ in range(reps)])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return P(torch.cuda.current_stream().cuda_stream)


def rand_rows(rng, n, width):
    return dev(rng.integers(0, 256, size=(n, width), dtype=np.uint8))


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s: %d %s" % (what, rc, _lib.load().gpbc_last_error()))


def elements(rng, n):
    """n ciphertext heads (u, v, w) in HBM: u = [k] g1, v = e^a, w = e^b for random scalars"""
    g1, g2 = (dev(x) for x in bn254.generators())
    e = bn254.pair_batch(g1, g2)
    base = e.expand(n, 384).contiguous().reshape(-1)
    u = bn254.g1_scalar_mul(g1, rand_rows(rng, n, 32).reshape(-1)).reshape(n, 64)
    v = bn254.gt_exp(base, rand_rows(rng, n, 32).reshape(-1)).reshape(n, 384)
    w = bn254.gt_exp(base, rand_rows(rng, n, 32).reshape(-1)).reshape(n, 384)
    return u, v, w


def transcript(lib, rng, n, reps):
    u, v, w = elements(rng, n)
    out_new, out_old = (torch.empty((n, 32), dtype=torch.uint8, device="cuda") for _ in range(2))
    enc_u, enc_v, enc_w = (torch.empty((n, width), dtype=torch.uint8, device="cuda") for width in (32, 384, 384))
    pin_u, pin_v, pin_w = (torch.empty((n, width), dtype=torch.uint8).pin_memory() for width in (32, 384, 384))
    pin_beta = torch.empty((n, 32), dtype=torch.uint8).pin_memory()

    def new():
        check(lib.gpbc_hash_g1_gt_gt_to_fr_dev(P(u.data_ptr()), P(v.data_ptr()), P(w.data_ptr()), n, P(out_new.data_ptr()), stream()), "hash_g1_gt_gt_to_fr_dev")

    def marshal():
        check(lib.gpbc_g1_marshal_batch_dev(P(u.data_ptr()), n, 1, P(enc_u.data_ptr()), stream()), "g1_marshal_batch_dev")
        check(lib.gpbc_gt_marshal_batch_dev(P(v.data_ptr()), n, P(enc_v.data_ptr()), stream()), "gt_marshal_batch_dev")
        check(lib.gpbc_gt_marshal_batch_dev(P(w.data_ptr()), n, P(enc_w.data_ptr()), stream()), "gt_marshal_batch_dev")
    parts = {}

    def old():
        t0 = time.perf_counter()
        marshal()
        pin_u.copy_(enc_u, non_blocking=True)
        pin_v.copy_(enc_v, non_blocking=True)
        pin_w.copy_(enc_w, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        bu, bv, bw = pin_u.numpy(), pin_v.numpy(), pin_w.numpy()
        sha, rows = hashlib.sha256, []
        for i in range(n):
            h = sha(bu[i])
            h.update(bv[i])
            h.update(bw[i])
            rows.append((int.from_bytes(h.digest(), "big") % R_ORDER).to_bytes(32, "little"))
        pin_beta.numpy()[...] = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(n, 32)
        t2 = time.perf_counter()
        out_old.copy_(pin_beta, non_blocking=True)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        parts.setdefault("marshal_and_copy_to_host_ms", []).append((t1 - t0) * 1e3)
        parts.setdefault("hashlib_and_reduce_ms", []).append((t2 - t1) * 1e3)
        parts.setdefault("copy_back_ms", []).append((t3 - t2) * 1e3)
    new()
    old()
    torch.cuda.synchronize()
    parts.clear()
    same = bool((out_new == out_old).all())
    t_new, t_dev, t_whole = [], [], []
    for _ in range(reps):                                                        # alternating, repetition by repetition
        t_new.append(timed(new))
        t_dev.append(timed(marshal))
        t_whole.append(wall(old))
    moved = n * (64 + 384 + 384 + 32)
    rec = {"n": n, "same_scalars": same, "hash_kernel": stats(t_new), "old_route_device_part_three_marshal_launches": stats(t_dev),
           "old_route_whole": stats(t_whole), "old_route_whole_parts": {k: stats(ts) for k, ts in parts.items()},
           "bytes_read_and_written_per_item": {"hash_kernel": 832 + 32, "three_marshal_launches": 832 + 800}}
    med = rec["hash_kernel"]["median_ms"]
    rec["hash_kernel"].update(M_items_per_s=n / med / 1e3, bytes_per_s=moved / med * 1e3, share_of_hbm_peak=moved / med * 1e3 / HBM_PEAK_BYTES_PER_S)
    rec["ratio_device_part_over_hash_kernel"] = rec["old_route_device_part_three_marshal_launches"]["median_ms"] / med
    rec["ratio_whole_over_hash_kernel"] = rec["old_route_whole"]["median_ms"] / med
    return rec


def plain_sha(lib, rng, n, length, reps):
    msgs = rand_rows(rng, n, length).reshape(-1)
    off = torch.arange(0, (n + 1) * length, length, dtype=torch.int64, device="cuda")
    out = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    rec = {"n": n, "message_bytes": length}
    for to_fr in (0, 1):
        r = measure(lambda: check(lib.gpbc_sha256_batch_dev(P(msgs.data_ptr()), P(off.data_ptr()), n * length, n, to_fr, P(out.data_ptr()), stream()), "sha256_batch_dev"), reps)
        r.update(M_messages_per_s=n / r["median_ms"] / 1e3, message_bytes_per_s=n * length / r["median_ms"] * 1e3)
        rec["scalars" if to_fr else "digests"] = r
    sample = [0, n // 2, n - 1]
    host = msgs.reshape(n, length)[sample].cpu().numpy()
    want = [(int.from_bytes(hashlib.sha256(row.tobytes()).digest(), "big") % R_ORDER).to_bytes(32, "little") for row in host]
    rec["sample_matches_hashlib"] = [bytes(out[i].cpu().numpy()) for i in sample] == want
    return rec


class StageTimer:
    """the engine with device events around every call: per entry name, the summed time of one planner run"""

    def __init__(self, engine):
        self._engine, self.events = engine, []

    def __getattr__(self, name):
        fn = getattr(self._engine, name)
        if not callable(fn):
            return fn

        def call(*args, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            res = fn(*args, **kw)
            e.record()
            self.events.append((name, s, e))
            return res
        return call

    def take(self):
        torch.cuda.synchronize()
        out = {}
        for name, s, e in self.events:
            out[name] = out.get(name, 0.0) + s.elapsed_time(e)
        self.events = []
        return out


def planner(rng, n, k, reps):
    g1, g2 = (dev(x) for x in bn254.generators())
    alpha = rand_rows(rng, 1, 32)
    h = bn254.g2_scalar_mul(g2, rand_rows(rng, k, 32).reshape(-1)).reshape(k, 128)
    g1_alpha = bn254.g1_scalar_mul(g1, alpha.reshape(-1))
    ids, r, s = rand_rows(rng, n, 32), rand_rows(rng, n * k, 32), rand_rows(rng, n, 32)
    e_gg, e_gh = gentry06.public_pairings(bn254, g1, g2, h)
    messages = bn254.gt_exp(e_gg.expand(n, 384).contiguous().reshape(-1), rand_rows(rng, n, 32).reshape(-1)).reshape(n, 384)
    keys, cts, back = [None], [None], [None]

    def keygen(engine=bn254):
        keys[0] = gentry06.keygen_batch(engine, alpha, h, ids, r)

    def encrypt(engine=bn254):
        cts[0] = gentry06.encrypt_batch(engine, g1_alpha, e_gg, e_gh, messages, ids, s)

    def decrypt(engine=bn254):
        back[0] = gentry06.decrypt_batch(engine, keys[0][:2], *cts[0])
    rec = {"identities": n, "k": k, "public_pairings": measure(lambda: gentry06.public_pairings(bn254, g1, g2, h), reps),
           "keygen_batch": measure(keygen, reps), "encrypt_batch": measure(encrypt, reps), "decrypt_batch": measure(decrypt, reps)}
    staged = StageTimer(bn254)
    rec["stages_ms"] = {}
    for name, fn in (("keygen_batch", keygen), ("encrypt_batch", encrypt), ("decrypt_batch", decrypt)):
        fn(staged)
        rec["stages_ms"][name] = staged.take()
    rec["messages_returned"] = bool((back[0][0] == messages).all()) and bool(back[0][1].all()) and bool(keys[0][2].all())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-log-n", type=int, default=20)
    ap.add_argument("--planner-log-n", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-planner", action="store_true")
    args = ap.parse_args()
    bn254.init(0)
    lib = _lib.load()
    doc = {"reps": args.reps, "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
           "transcript_hash": {}, "sha256": {}, "gentry06": {}}
    rng = np.random.default_rng(2006)
    for log_n in sorted({min(16, args.max_log_n), args.max_log_n}):
        rec = transcript(lib, rng, 1 << log_n, args.reps)
        doc["transcript_hash"]["2^%d" % log_n] = rec
        print("H(u, v, w) n = 2^%d: kernel %.3f ms (%.1f M items/s, %.2f TB/s = %.0f %% of the HBM peak); the three marshal launches %.3f ms (%.2fx); the old route whole %.1f ms (%.0fx); same scalars %s" % (
            log_n, rec["hash_kernel"]["median_ms"], rec["hash_kernel"]["M_items_per_s"], rec["hash_kernel"]["bytes_per_s"] / 1e12, 100 * rec["hash_kernel"]["share_of_hbm_peak"],
            rec["old_route_device_part_three_marshal_launches"]["median_ms"], rec["ratio_device_part_over_hash_kernel"], rec["old_route_whole"]["median_ms"],
            rec["ratio_whole_over_hash_kernel"], rec["same_scalars"]), flush=True)
        torch.cuda.empty_cache()
        for length in (32, 1024):
            rec = plain_sha(lib, rng, 1 << log_n, length, args.reps)
            doc["sha256"]["%d B 2^%d" % (length, log_n)] = rec
            print("SHA-256 of %d-byte messages n = 2^%d: digests %.3f ms (%.1f M messages/s, %.2f GB/s), scalars %.3f ms; sample matches hashlib %s" % (
                length, log_n, rec["digests"]["median_ms"], rec["digests"]["M_messages_per_s"], rec["digests"]["message_bytes_per_s"] / 1e9, rec["scalars"]["median_ms"],
                rec["sample_matches_hashlib"]), flush=True)
            torch.cuda.empty_cache()
    if not args.skip_planner:
        n = 1 << min(args.planner_log_n, args.max_log_n)
        for k in (1, 3):
            rec = planner(rng, n, k, args.reps)
            doc["gentry06"]["k=%d" % k] = rec
            print("gentry06 k = %d at %d identities: keygen %.2f ms, encrypt %.2f ms, decrypt %.2f ms; messages returned %s" % (
                k, n, rec["keygen_batch"]["median_ms"], rec["encrypt_batch"]["median_ms"], rec["decrypt_batch"]["median_ms"], rec["messages_returned"]), flush=True)
            print("  stages (ms): %s" % json.dumps({p: {c: round(t, 3) for c, t in st.items()} for p, st in rec["stages_ms"].items()}), flush=True)
            lib.gpbc_release_workspaces()
            torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text if not args.out else "written to " + args.out)


if __name__ == "__main__":
    main()
