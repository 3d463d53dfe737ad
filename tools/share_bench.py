"""Secret sharing in Fr (gpbc_fr_poly_eval_dev, gpbc_fr_share_tree_dev: include/gpbc_bn254_share.h) on HBM-resident data against the
routes the engine had before them to the same bytes, and the two planners built on them:

  * fr_poly_eval at 2^16 x (d = 16, m = 24) and 2^12 x (d = 256, m = 256) against Horner by d - 1 rounds of gpbc_fr_mul_batch_dev +
    gpbc_fr_add_batch_dev over the k m elements (the coefficient columns are spread over the points before the clock starts, in that
    route's favour);
  * fr_share_tree at 2^16 items x {256-of-256, 128-of-256, 16 x (16-of-16) under 16-of-16} against the same tree gate level by gate
    level with fr_poly_eval and torch concatenations, and at 2^8 items against the recursion in Python integers (the ratio at that size);
  * bsw07.encrypt_batch at 2^16 ciphertexts x 256 leaves under the three policies, with the stages timed one by one, then
    bsw07.decrypt_batch_arrays on what it made (for 128-of-256 with a key that holds exactly 128 of the attributes);
  * sw05.keygen_batch / keygen_batch_large at 2^16 users x 32 attributes, d = 16.
Seeded inputs; the legs of a comparison alternate inside one repetition loop; the output bytes of the routes are compared before any
time is reported; device events.  One process, one device.  Writes one JSON document (profiles/secret_sharing.json records a run), and
rewrites it after every section.

    python tools/share_bench.py [--reps 5] [--log-n 16] [--out FILE] [--skip-planners] [--skip-large]"""
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

from gopairingbasedcryptography_amd import bn254, bsw07, sw05  # noqa: E402
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
    return dev(rng.integers(0, 256, size=shape + (32,), dtype=np.uint8))


def small_scalars(values):
    return dev(np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32).copy())


# ------------------------------------------------------------------------------------------------ policies
def flat_gate(k, n, first=0):
    return bsw07.Threshold(k, *[bsw07.Leaf(first + i) for i in range(n)])


POLICIES = {"256-of-256": lambda: flat_gate(256, 256), "128-of-256": lambda: flat_gate(128, 256),
            "16x(16-of-16) under 16-of-16": lambda: bsw07.Threshold(16, *[flat_gate(16, 16, 16 * g) for g in range(16)])}


def composed_tree(name, secrets, coeffs, k):
    """the same shares gate level by gate level: rows [value | coefficients] through fr_poly_eval at the shared points 1 .. n"""
    if name != "16x(16-of-16) under 16-of-16":
        t = 256 if name == "256-of-256" else 128
        rows = torch.cat([secrets.reshape(k, 1, 32), coeffs.reshape(k, t - 1, 32)], 1)
        return bn254.fr_poly_eval(rows.reshape(-1), POINTS[256].reshape(-1), t, 256)
    q = coeffs.reshape(k, 17, 15, 32)
    top = bn254.fr_poly_eval(torch.cat([secrets.reshape(k, 1, 32), q[:, 0]], 1).reshape(-1), POINTS[16].reshape(-1), 16, 16)               # [k, 16, 32]
    rows = torch.cat([top.reshape(k * 16, 1, 32), q[:, 1:].reshape(k * 16, 15, 32)], 1)
    return bn254.fr_poly_eval(rows.reshape(-1), POINTS[16].reshape(-1), 16, 16).reshape(k, 256, 32)


POINTS = {}


def python_share(node, secret, it, out):
    """AccessTreeNode.ShareSecret in Python integers"""
    if isinstance(node, bsw07.Leaf):
        out.append(secret)
        return
    q = [secret] + [next(it) for _ in range(node.k - 1)]
    for i, c in enumerate(node.children, start=1):
        v = 0
        for cf in reversed(q):
            v = (v * i + cf) % R
        python_share(c, v, it, out)


def ints(t):
    return [int.from_bytes(r.tobytes(), "little") for r in t.cpu().numpy().reshape(-1, 32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-planners", action="store_true")
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    bn254.init(0)
    rng = np.random.default_rng(2007)
    n = 1 << args.log_n
    doc = {"reps": args.reps, "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "log_n": args.log_n, "poly_eval": {}, "share_tree": {}}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
    POINTS[256], POINTS[16] = small_scalars(range(1, 257)), small_scalars(range(1, 17))

    # ---- polynomial evaluation
    for k, d, m in ((n, 16, 24), (max(n >> 4, 1), 256, 256)):
        coeffs, points = rand_scalars(rng, k, d), rand_scalars(rng, k, m)
        out = torch.empty((k, m, 32), dtype=torch.uint8, device="cuda")
        spread = [coeffs[:, i:i + 1].expand(k, m, 32).contiguous().reshape(-1) for i in range(d)]       # before the clock: in the composed route's favour
        flat_points, acc = points.reshape(-1), torch.empty(k * m * 32, dtype=torch.uint8, device="cuda")

        def new():
            bn254.fr_poly_eval(coeffs.reshape(-1), flat_points, d, m, out=out)

        def composed():
            bn254.fr_mul(spread[d - 1], flat_points, out=acc)
            for i in range(d - 2, 0, -1):
                bn254.fr_add(acc, spread[i], out=acc)
                bn254.fr_mul(acc, flat_points, out=acc)
            bn254.fr_add(acc, spread[0], out=acc)
        new()
        composed()
        torch.cuda.synchronize()
        rec = {"k": k, "d": d, "m": m, "horner_steps": k * m * (d - 1), "same_bytes": bool((acc == out.reshape(-1)).all())}
        rec.update(alternate({"fr_poly_eval": new, "composed_fr_mul_fr_add": composed}, args.reps))
        rec["G_steps_per_s"] = rec["horner_steps"] / rec["fr_poly_eval"]["median_ms"] / 1e6
        rec["ratio_composed_over_kernel"] = rec["composed_fr_mul_fr_add"]["median_ms"] / rec["fr_poly_eval"]["median_ms"]
        doc["poly_eval"]["%d x (d=%d, m=%d)" % (k, d, m)] = rec
        print("fr_poly_eval %d x (%d, %d): %.3f ms = %.1f G steps/s; composed %.3f ms (%.1fx); same bytes %s" % (
            k, d, m, rec["fr_poly_eval"]["median_ms"], rec["G_steps_per_s"], rec["composed_fr_mul_fr_add"]["median_ms"], rec["ratio_composed_over_kernel"], rec["same_bytes"]), flush=True)
        del spread, acc, out, coeffs, points
        torch.cuda.empty_cache()
        save()

    # ---- sharing over a tree
    trees = {}
    for name, make in POLICIES.items():
        tree = make()
        nodes, attrs = bsw07.share_plan(tree)
        h = bn254.ShareTree(nodes)
        trees[name] = (tree, nodes, attrs)
        secrets, coeffs = rand_scalars(rng, n), rand_scalars(rng, n, h.coeffs)
        out = torch.empty((n, h.leaves, 32), dtype=torch.uint8, device="cuda")
        got = [None]

        def new():
            h.share(secrets.reshape(-1), coeffs.reshape(-1), out=out)

        def composed():
            got[0] = composed_tree(name, secrets, coeffs, n)
        new()
        composed()
        torch.cuda.synchronize()
        steps = n * (256 * (255 if name == "256-of-256" else 127) if "under" not in name else 17 * 16 * 15)
        rec = {"items": n, "leaves": h.leaves, "coeffs_per_item": h.coeffs, "horner_steps": steps, "same_bytes": bool((got[0].reshape(-1) == out.reshape(-1)).all())}
        rec.update(alternate({"fr_share_tree": new, "composed_levels_fr_poly_eval": composed}, args.reps))
        rec["G_steps_per_s"] = steps / rec["fr_share_tree"]["median_ms"] / 1e6
        rec["ratio_composed_over_kernel"] = rec["composed_levels_fr_poly_eval"]["median_ms"] / rec["fr_share_tree"]["median_ms"]
        # 2^8 items against Python integers
        k8 = min(256, n)
        s8, q8 = ints(secrets[:k8]), ints(coeffs[:k8])
        t0 = time.perf_counter()
        want = []
        for j in range(k8):
            python_share(tree, s8[j], iter(q8[j * h.coeffs:(j + 1) * h.coeffs]), want)
        py_ms = (time.perf_counter() - t0) * 1e3
        small = alternate({"kernel": lambda: h.share(secrets[:k8].reshape(-1), coeffs[:k8].reshape(-1), out=out[:k8])}, args.reps)["kernel"]
        rec["python_integers_at_256_items"] = {"items": k8, "python_ms": py_ms, "kernel": small, "same_values": ints(out[:k8]) == [v % R for v in want],
                                               "ratio_python_over_kernel": py_ms / small["median_ms"]}
        doc["share_tree"][name] = rec
        print("fr_share_tree %s x %d: %.3f ms = %.1f G steps/s; level by level %.3f ms (%.2fx); same bytes %s; %d items in Python %.0f ms vs %.3f ms, same %s" % (
            name, n, rec["fr_share_tree"]["median_ms"], rec["G_steps_per_s"], rec["composed_levels_fr_poly_eval"]["median_ms"], rec["ratio_composed_over_kernel"], rec["same_bytes"],
            k8, py_ms, small["median_ms"], rec["python_integers_at_256_items"]["same_values"]), flush=True)
        h.close()
        del secrets, coeffs, out, got
        torch.cuda.empty_cache()
        save()

    if not args.skip_planners:
        # ---- BSW07 Encrypt, then Decrypt of what it made
        g1, g2 = (dev(x) for x in bn254.generators())
        sc = lambda: int.from_bytes(rng.integers(0, 256, size=32, dtype=np.uint8).tobytes(), "little") % R
        alpha, beta, r = sc(), sc(), sc()
        e = bn254.pair_batch(g1, g2)
        e_alpha = bn254.gt_exp(e.reshape(-1), small_scalars([alpha]).reshape(-1)).reshape(-1)
        hpk = bn254.g1_scalar_mul(g1, small_scalars([beta]).reshape(-1)).reshape(-1)
        hj = [sc() for _ in range(256)]
        H1 = bn254.g1_scalar_mul(g1, small_scalars(hj).reshape(-1)).reshape(256, 64).cpu().numpy()
        H2 = bn254.g2_scalar_mul(g2, small_scalars(hj).reshape(-1)).reshape(256, 128)
        rj = [sc() for _ in range(256)]
        g2r = bn254.g2_scalar_mul(g2, small_scalars([r]).reshape(-1)).reshape(1, 128)
        Dj = bn254.g2_add(g2r.expand(256, 128).contiguous().reshape(-1), bn254.g2_scalar_mul(H2.reshape(-1), small_scalars(rj).reshape(-1)).reshape(-1)).reshape(256, 128).cpu().numpy()
        Djp = bn254.g2_scalar_mul(g2, small_scalars(rj).reshape(-1)).reshape(256, 128).cpu().numpy()
        D = bn254.g2_scalar_mul(g2, small_scalars([(alpha + r) * pow(beta, -1, R) % R]).reshape(-1)).reshape(-1).cpu().numpy()
        messages = bn254.gt_exp(e.expand(n, 384).contiguous().reshape(-1), rand_scalars(rng, n).reshape(-1)).reshape(n, 384)
        h1 = {a: H1[a] for a in range(256)}
        doc["bsw07_encrypt"] = {}
        for name, (tree, nodes, attrs) in trees.items():
            plan = (nodes, attrs)
            s, coeffs = rand_scalars(rng, n), rand_scalars(rng, n, sum(t - 1 for _, t in nodes if t))
            ct = [None]

            def encrypt():
                ct[0] = bsw07.encrypt_batch(bn254, plan, hpk, e_alpha, h1, messages, s, coeffs)
            handle = bn254.ShareTree(nodes)
            shares = handle.share(s.reshape(-1), coeffs.reshape(-1)).reshape(-1)
            hy = dev(np.stack([H1[a] for a in attrs])).reshape(1, 256, 64).expand(n, 256, 64).contiguous().reshape(-1)
            base = e_alpha.reshape(1, 384).expand(n, 384).contiguous().reshape(-1)
            rec = alternate({"encrypt_batch": encrypt, "sharing": lambda: handle.share(s.reshape(-1), coeffs.reshape(-1)),
                             "generator_multiplications": lambda: bn254.g1_scalar_mul_base(shares), "h1_multiplications": lambda: bn254.g1_scalar_mul(hy, shares),
                             "c": lambda: bn254.g1_scalar_mul(hpk, s.reshape(-1)), "gt_exp_and_mul": lambda: bn254.gt_mul(bn254.gt_exp(base, s.reshape(-1)), messages.reshape(-1))}, args.reps)
            handle.close()
            del shares, hy, base
            torch.cuda.empty_cache()
            held = set(range(256)) if name != "128-of-256" else set(range(0, 256, 2))           # exactly 128 of the attributes
            short = bsw07.decrypt_plan(tree, held - {max(held)})
            dplan = bsw07.decrypt_plan(tree, held)
            folded = bsw07.fold_key(bn254, dplan, {a: Dj[a] for a in held}, {a: Djp[a] for a in held})
            cols = dev(np.array([i - 1 for i in folded[0]], dtype=np.int64))
            c_tilde, c, cy, cy_prime = ct[0]
            cy, cy_prime = cy.index_select(1, cols).contiguous(), cy_prime.index_select(1, cols).contiguous()
            back = [None]

            def decrypt():
                back[0] = bsw07.decrypt_batch_arrays(bn254, folded, D, c_tilde, c, cy, cy_prime)
            rec["decrypt_batch_arrays"] = alternate({"decrypt": decrypt}, max(1, args.reps // 2))["decrypt"]
            rec.update({"ciphertexts": n, "leaves": 256, "attributes_held": len(held), "leaves_used": len(folded[0]), "one_attribute_short_has_no_plan": short is None,
                        "all_messages_recovered": bool((back[0].reshape(n, 384) == messages).all())})
            doc["bsw07_encrypt"][name] = rec
            print("bsw07.encrypt_batch %s x %d: %.1f ms (sharing %.2f, generator %.1f, H1 %.1f, C %.1f, GT %.1f); decrypt with %d leaves %.1f ms, all messages recovered %s" % (
                name, n, rec["encrypt_batch"]["median_ms"], rec["sharing"]["median_ms"], rec["generator_multiplications"]["median_ms"], rec["h1_multiplications"]["median_ms"],
                rec["c"]["median_ms"], rec["gt_exp_and_mul"]["median_ms"], len(folded[0]), rec["decrypt_batch_arrays"]["median_ms"], rec["all_messages_recovered"]), flush=True)
            del ct, back, cy, cy_prime, c_tilde, c, s, coeffs
            torch.cuda.empty_cache()
            bn254.release_workspaces()
            save()
        del messages

        # ---- SW05 KeyGenerate
        k, m, d = n, 32, 16
        coeffs, attrs, side = rand_scalars(rng, k, d - 1), rand_scalars(rng, k, m), rand_scalars(rng, k, m)
        y = sc()
        legs = {"keygen_batch": lambda: sw05.keygen_batch(bn254, y, coeffs, attrs, side),
                "fr_poly_eval_alone": lambda: bn254.fr_poly_eval(torch.cat([small_scalars([y]).reshape(1, 1, 32).expand(k, 1, 32), coeffs], 1).reshape(-1), attrs.reshape(-1), d, m)}
        table = None
        if not args.skip_large:
            n_univ = 32
            taus = small_scalars([sc() for _ in range(n_univ + 1)])
            table = bn254.FixedBase(torch.cat([g2.reshape(1, 128), bn254.g2_scalar_mul(g2, taus.reshape(-1)).reshape(-1, 128)]).contiguous(), g2=True)
            legs["keygen_batch_large"] = lambda: sw05.keygen_batch_large(bn254, table, n_univ, y, coeffs, attrs, side)
            legs["compute_t_alone"] = lambda: sw05.compute_t(bn254, table, n_univ, attrs.reshape(k * m, 32))
        rec = alternate(legs, max(1, args.reps // 2))
        rec.update({"users": k, "attributes": m, "d": d})
        doc["sw05_keygen"] = rec
        print("sw05 keygen %d users x %d attributes, d = %d: " % (k, m, d) + ", ".join("%s %.1f ms" % (name, rec[name]["median_ms"]) for name in legs), flush=True)
        if table is not None:
            table.close()
        save()
    print(json.dumps(doc, indent=1) if not args.out else "written to " + args.out)


if __name__ == "__main__":
    main()
