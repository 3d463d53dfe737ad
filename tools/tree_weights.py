"""Threshold-tree reconstruction weights (gpbc_fr_tree_weights_dev: include/gpbc_bn254_recon.h) and bsw07.decrypt_batch_keys on HBM-resident
data:

  1. ShareTree.weights at 2^16 items x {256-of-256, 128-of-256, 16 x (16-of-16) under 16-of-16}, with gpbc_fr_inverse_batch_dev on as many
     elements (items x leaves) beside it; sum_y w_y share_y = secret is checked on the device for every item first;
  2. bsw07.decrypt_batch_keys at 2^12 (key, ciphertext) items x 256 leaves under the three policies, stage by stage;
  3. the comparison at 256 items: the only route to the same messages without the kernel — bsw07.decrypt_plan per item in Python integers,
     the weights uploaded, then the identical engine calls — beside decrypt_batch_keys, messages equal byte for byte.  The ratio is that
     of this size.
Keys are one master key (one r) restricted to each user's attribute set, which is a valid key of that set; ciphertexts come from
bsw07.encrypt_batch.  Seeded inputs; medians of --reps repetitions between device events (the planner, which waits for the stream once,
between host clocks around a synchronize; the Python route of 3. once).  One process, one device.  Writes one JSON document
(profiles/tree_weights.json records a run) and rewrites it after every section.

    python tools/tree_weights.py [--reps 5] [--log-n 16] [--log-keys 12] [--parent COMMIT] [--out FILE]"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gopairingbasedcryptography_amd import bn254, bsw07  # noqa: E402
from gopairingbasedcryptography_amd._buffers import R_ORDER as R  # noqa: E402


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


def alternate(legs, reps, clock=timed):
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            ts[name].append(clock(fn))
    return {name: stats(t) for name, t in ts.items()}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rand_scalars(rng, *shape):
    return dev(rng.integers(0, 256, size=shape + (32,), dtype=np.uint8))


def small_scalars(values):
    return dev(np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32).copy())


def flat_gate(k, n, first=0):
    return bsw07.Threshold(k, *[bsw07.Leaf(first + i) for i in range(n)])


POLICIES = {"256-of-256": lambda: flat_gate(256, 256), "128-of-256": lambda: flat_gate(128, 256),
            "16x(16-of-16) under 16-of-16": lambda: bsw07.Threshold(16, *[flat_gate(16, 16, 16 * g) for g in range(16)])}


def held_sets(name, n, rng):
    """[n, 256] uint8: what user t holds.  128-of-256: about 160 random attributes (at least 128, so the first 128 held are used) with
    every eighth user at 127 (not satisfied); the two all-of policies: everything, every eighth user one attribute short."""
    if name == "128-of-256":
        held = np.zeros((n, 256), dtype=np.uint8)
        for t in range(n):
            count = 127 if t % 8 == 7 else int(rng.integers(128, 193))
            held[t, rng.permutation(256)[:count]] = 1
        return held
    held = np.ones((n, 256), dtype=np.uint8)
    short = np.arange(7, n, 8)
    held[short, rng.integers(0, 256, size=len(short))] = 0
    return held


class HostWeights:
    """bn254 with ShareTree.weights from bsw07.decrypt_plan in Python integers, an item at a time: the route without the kernel"""

    class Tree:
        def __init__(self, outer, nodes):
            self.outer, self.leaves = outer, sum(1 for _, t in nodes if not t)

        def weights(self, held):
            h = held.cpu().numpy().reshape(-1, self.leaves)
            t0 = time.perf_counter()
            w, ok = np.zeros((len(h), self.leaves, 32), dtype=np.uint8), np.zeros(len(h), dtype=np.uint8)
            for j, row in enumerate(h):
                plan = bsw07.decrypt_plan(self.outer.tree, {self.outer.attrs[y] for y in np.nonzero(row)[0]})
                if plan is not None:
                    ok[j] = 1
                    for leaf_id, (_, delta) in plan.items():
                        w[j, leaf_id - 1] = np.frombuffer(int(delta).to_bytes(32, "little"), dtype=np.uint8)
            self.outer.python_ms.append((time.perf_counter() - t0) * 1e3)
            return dev(w), dev(ok)

        def close(self):
            pass

    def __init__(self, tree, attrs):
        self.tree, self.attrs, self.python_ms = tree, attrs, []

    def ShareTree(self, nodes):
        return HostWeights.Tree(self, nodes)

    def __getattr__(self, name):
        return getattr(bn254, name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--log-keys", type=int, default=12)
    ap.add_argument("--parent", default=None, help="the commit this tree was built on (recorded in the document)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bn254.init(0)
    rng = np.random.default_rng(2011)
    n, nk = 1 << args.log_n, 1 << args.log_keys
    doc = {"reps": args.reps, "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "parent_commit": args.parent, "log_n": args.log_n,
           "log_keys": args.log_keys, "tree_weights": {}, "decrypt_batch_keys": {}, "at_256_items": {}}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")

    # ---- 1. the kernel
    for name, make in POLICIES.items():
        nodes, _ = bsw07.share_plan(make())
        h = bn254.ShareTree(nodes)
        held = dev(held_sets(name, n, rng))
        w, ok = torch.empty((n, 256, 32), dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
        h.weights(held.reshape(-1), out=w, ok_out=ok)
        # the weights recombine the shares of random secrets
        secrets, coeffs = rand_scalars(rng, n), rand_scalars(rng, n, h.coeffs)
        prod = bn254.fr_mul(w.reshape(-1), h.share(secrets.reshape(-1), coeffs.reshape(-1)).reshape(-1)).reshape(n, 256, 32)
        m = 256
        while m > 1:
            m //= 2
            prod = bn254.fr_add(prod[:, :m].contiguous().reshape(-1), prod[:, m:2 * m].contiguous().reshape(-1)).reshape(n, m, 32)
        want = bn254.fr_mul(secrets.reshape(-1), small_scalars([1]).reshape(-1)).reshape(n, 32) * ok.reshape(n, 1)
        rec = {"items": n, "leaves": 256, "satisfied": int(ok.sum().item()), "weights_recombine_the_shares": bool((prod.reshape(n, 32) == want).all().item()),
               "used_leaves": int((w != 0).any(2).sum().item())}
        del prod, secrets, coeffs, want
        elements = rand_scalars(rng, n * 256).reshape(-1)
        inv = torch.empty_like(elements)
        rec.update(alternate({"tree_weights": lambda: h.weights(held.reshape(-1), out=w, ok_out=ok), "fr_inverse_same_elements": lambda: bn254.fr_inverse(elements, out=inv)}, args.reps))
        rec["ns_per_used_leaf"] = rec["tree_weights"]["median_ms"] * 1e6 / max(rec["used_leaves"], 1)
        doc["tree_weights"][name] = rec
        print("tree_weights %s x %d: %.3f ms (%d satisfied, %d used leaves, %.1f ns each); fr_inverse on %d elements %.3f ms; recombines %s" % (
            name, n, rec["tree_weights"]["median_ms"], rec["satisfied"], rec["used_leaves"], rec["ns_per_used_leaf"], n * 256, rec["fr_inverse_same_elements"]["median_ms"],
            rec["weights_recombine_the_shares"]), flush=True)
        h.close()
        del held, w, ok, elements, inv
        torch.cuda.empty_cache()
        save()

    # ---- 2. and 3. the planner
    g1, g2 = (dev(x) for x in bn254.generators())
    sc = lambda: int.from_bytes(rng.integers(0, 256, size=32, dtype=np.uint8).tobytes(), "little") % R
    alpha, beta, r = sc(), sc(), sc()
    e = bn254.pair_batch(g1, g2)
    e_alpha = bn254.gt_exp(e.reshape(-1), small_scalars([alpha]).reshape(-1)).reshape(-1)
    hpk = bn254.g1_scalar_mul(g1, small_scalars([beta]).reshape(-1)).reshape(-1)
    hj, rj = [sc() for _ in range(256)], [sc() for _ in range(256)]
    H1 = bn254.g1_scalar_mul(g1, small_scalars(hj).reshape(-1)).reshape(256, 64).cpu().numpy()
    Dj = bn254.g2_scalar_mul(g2, small_scalars([(r + a * b) % R for a, b in zip(hj, rj)]).reshape(-1)).reshape(1, 256, 128)          # g2^r H2(a)^rj, H2(a) = [h_a] g2
    Djp = bn254.g2_scalar_mul(g2, small_scalars(rj).reshape(-1)).reshape(1, 256, 128)
    D = bn254.g2_scalar_mul(g2, small_scalars([(alpha + r) * pow(beta, -1, R) % R]).reshape(-1)).reshape(-1).cpu().numpy()
    messages = bn254.gt_exp(e.expand(nk, 384).contiguous().reshape(-1), rand_scalars(rng, nk).reshape(-1)).reshape(nk, 384)
    h1 = {a: H1[a] for a in range(256)}
    dj, djp = Dj.expand(nk, 256, 128).contiguous(), Djp.expand(nk, 256, 128).contiguous()
    for name, make in POLICIES.items():
        tree = make()
        plan = bsw07.share_plan(tree)
        nodes, attrs = plan
        s, coeffs = rand_scalars(rng, nk), rand_scalars(rng, nk, sum(t - 1 for _, t in nodes if t))
        c_tilde, c, cy, cyp = bsw07.encrypt_batch(bn254, plan, hpk, e_alpha, h1, messages, s, coeffs)
        held_host = held_sets(name, nk, rng)
        held = dev(held_host)
        got = [None]

        def decrypt(k=nk, engine=bn254):
            got[0] = bsw07.decrypt_batch_keys(engine, plan, held[:k], D, dj[:k], djp[:k], c_tilde[:k], c[:k], cy[:k], cyp[:k])
        decrypt()
        msgs, ok = got[0]
        rec = {"items": nk, "leaves": 256, "satisfied": int(ok.sum().item()),
               "every_satisfied_message_recovered": bool((msgs == messages * ok.reshape(nk, 1)).all().item()), "unsatisfied_rows_zero": bool((msgs[ok == 0] == 0).all().item())}
        # the stages on their own, on the lists the planner builds
        handle = bn254.ShareTree(nodes)
        w, _ = handle.weights(held.reshape(-1))
        good = np.nonzero(ok.cpu().numpy())[0]
        index, mask, U = bsw07.used_columns((w.reshape(nk * 256, 32) != 0).any(1).cpu().numpy().reshape(nk, 256)[good])
        flat_index, keep, ng = dev((good[:, None] * 256 + index).reshape(-1)), dev(mask.reshape(-1, 1)), len(good)
        gather = lambda a, width: (a.reshape(nk * 256, width).index_select(0, flat_index) * keep).reshape(ng, U, width)
        wg = gather(w, 32)
        scalars = torch.cat([wg, bn254.fr_neg(wg.reshape(-1)).reshape(ng, U, 32)], 1).contiguous()
        bases = torch.cat([gather(cy, 64), gather(cyp, 64)], 1).contiguous()
        folded = bn254.g1_scalar_mul(bases.reshape(-1), scalars.reshape(-1)).reshape(ng, 2 * U, 64)
        neg_d = dev(bn254.g2_neg(D)).reshape(1, 1, 128).expand(ng, 1, 128)
        P = torch.cat([folded, c[dev(good)].reshape(ng, 1, 64)], 1).contiguous()
        Q = torch.cat([gather(dj, 128), gather(djp, 128), neg_d], 1).contiguous()
        seg = np.arange(0, ng * (2 * U + 1) + 1, 2 * U + 1, dtype=np.uint64)
        X = bn254.multi_pair(P.reshape(-1), Q.reshape(-1), seg)
        rec.update({"used_columns_U": U, "pairs_per_item": 2 * U + 1, "pairs_without_compaction": 2 * 256 + 1})
        rec["stages"] = alternate({"tree_weights": lambda: handle.weights(held.reshape(-1)), "fr_neg": lambda: bn254.fr_neg(wg.reshape(-1)),
                                   "gathers": lambda: (gather(w, 32), gather(cy, 64), gather(cyp, 64), gather(dj, 128), gather(djp, 128)),
                                   "g1_scalar_mul": lambda: bn254.g1_scalar_mul(bases.reshape(-1), scalars.reshape(-1)),
                                   "multi_pair": lambda: bn254.multi_pair(P.reshape(-1), Q.reshape(-1), seg), "gt_mul": lambda: bn254.gt_mul(c_tilde[dev(good)].reshape(-1), X.reshape(-1))},
                                  max(1, args.reps // 2))
        handle.close()
        del w, wg, scalars, bases, folded, P, Q, X
        torch.cuda.empty_cache()
        rec["decrypt_batch_keys"] = alternate({"whole": decrypt}, max(1, args.reps // 2), clock=wall)["whole"]
        doc["decrypt_batch_keys"][name] = rec
        print("decrypt_batch_keys %s x %d: %.1f ms whole (U = %d: %s); %d satisfied, recovered %s" % (
            name, nk, rec["decrypt_batch_keys"]["median_ms"], U, ", ".join("%s %.2f" % (k, v["median_ms"]) for k, v in rec["stages"].items()), rec["satisfied"],
            rec["every_satisfied_message_recovered"]), flush=True)
        save()

        # ---- 3. 256 items: decrypt_plan per item in Python, then the identical engine calls
        k8 = min(256, nk)
        host_engine = HostWeights(tree, attrs)
        python_route_ms = wall(lambda: decrypt(k8, host_engine))                        # once: seconds of host arithmetic, nothing to take a median of
        by_python = got[0][0].clone()
        kernel_route = alternate({"decrypt_batch_keys": lambda: decrypt(k8)}, 3, clock=wall)["decrypt_batch_keys"]
        same = bool((got[0][0] == by_python).all().item())
        doc["at_256_items"][name] = {"items": k8, "messages_equal_byte_for_byte": same, "python_decrypt_plan_then_engine_ms": python_route_ms,
                                     "of_which_python_weights_ms": host_engine.python_ms[0], "decrypt_batch_keys": kernel_route,
                                     "ratio_python_route_over_kernel_route": python_route_ms / kernel_route["median_ms"]}
        print("  at %d items: decrypt_plan per item + engine %.1f ms (the Python weights %.1f ms), decrypt_batch_keys %.1f ms: %.1fx; messages equal %s" % (
            k8, python_route_ms, host_engine.python_ms[0], kernel_route["median_ms"], doc["at_256_items"][name]["ratio_python_route_over_kernel_route"], same), flush=True)
        del c_tilde, c, cy, cyp, s, coeffs, held
        torch.cuda.empty_cache()
        bn254.release_workspaces()
        save()
    print(json.dumps(doc, indent=1) if not args.out else "written to " + args.out)


if __name__ == "__main__":
    main()
