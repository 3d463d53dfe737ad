#!/usr/bin/env python3
"""Headline benchmark: BN254 pairings/s (+ G1/G2 scalar-mults/s) at batch 2^20 per MI355X  (BASELINE.json).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One step = one pass of the hot path over one batch: B independent bn254.Pair calls (Miller-loop kernels +
final-exponentiation kernel) on synthetic random points P_i=[k("P",i)]g1, Q_i=[k("Q",i)]g2,
inputs and outputs resident in HBM.  Each rank owns its own batch of B pairs (weak scaling, no data-path
collective: SURVEY.md §8e); value = pairs all ranks processed / max-over-ranks time.

A plain run only sets up, warms up, times the K steps and prints the headline line.  --dump-outputs DIR then writes a
fixed, seeded sample of rank 0's GT values from the last timed step (the bytes a caller of the path receives, one float32
per byte, exact) as DIR/pair_gt.npy, and the batch indices of its rows as DIR/pair_gt_index.npy: the inputs are the same
from run to run, so two builds can be compared output for output.  --full adds everything below: every rank bit-compares
a sample of its own outputs with the oracle and the run fails if any rank disagrees, and these objects join the line
(--no-secondary, --no-configs, --no-cpu and --no-scalar-mul trim them):
  roofline     the single kernel with the largest time per step (rocprofv3 agrees: profiles/) against the VALU integer-MAC
               roofline: algorithmic MACs per launch (nominal Fp-mul x 136 MAC x pairs) / its mean duration
               from HIP events on the launch stream (gpbc_profile_begin / _end bracket every launch).  peak = measured
               v_mad_u64_u32 issue rate of one MI355X (profiles/r01_microbench_valu.txt).  bound is "valu": this path is
               carry-chain integer work, neither HBM- nor MFMA-bound.  `kernels` has every kernel of the step (time, launches,
               fraction), `stages` the Miller stage and the final exponentiation, `traffic` the HBM bytes of ALL kernels of
               one step from the committed rocprofv3 --pmc passes (profiles/pmc_traffic.json) beside the algorithmic bytes.
  cpu_baseline the C restatement (oracle/, "port") timed on all host cores this process may use, rank 0, N=1 only, bounded
               sample; cpu_baseline_1core the same on one thread; actual_fp_mul its instrumented Fp-mul counts.
  value_pcie_inclusive  the host-pointer entry gpbc_pair_batch on the same batch (upload + kernels + download).
  roofline.scalar_mul   the other half of the metric: G1 and G2 scalar-mults/s at the same batch, each with its kernel's time from
               the same HIP-event bracket, the nominal (2 500 / 7 500 Fp-mul x 136 MAC) and executed-MAD fractions.
  concurrent_calls      calls/s of T = 1, 8, 64 OS threads looping ONE-element host-pointer calls (the reference's call shape; native
               harness tools/concurrent_calls.cpp over the C ABI, every result compared); a compact copy sits in cpu_baseline beside
               the port's rates.
  secondary    wire / hash-to-curve / fixed-base / GT.Exp rates, and `configs`: BASELINE configs
               2-4 at their stated sizes (aggregate verification of 2^20 signatures, BSW07 decrypt of 2^16 ciphertexts under
               both 256-attribute policies, AFP25 batch decryption of 2^18 identities), each timed and checked; with N > 1
               they shard over the ranks and run their all-gather through the library's own RCCL communicator.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import bench_workloads as wl                 # noqa: E402  (synthetic inputs of SURVEY.md §8d)

MAC_PER_FP_MUL = 136                      # 8x32-bit CIOS: 64 product + 64 reduction + 8
FP_MUL_MILLER, FP_MUL_FINAL_EXP, FP_MUL_G1, FP_MUL_G2 = 7000, 5000, 2500, 7500   # nominal, fixed for grading
# nominal split of the Miller loop between its two kernels, from SURVEY §8a-1's per-step figures (point doubling + line ~28
# of ~99 Fp-mul per doubling step): 2000 for the line phase, 5000 for the Fp12 accumulator
NOMINAL_FP_MUL = {"k_miller_lines": 2000, "k_miller_accumulate": 5000, "k_final_exp": FP_MUL_FINAL_EXP}
EXECUTED_MAD = {}                         # filled from profiles/executed_mads.json (tests/test_device_math_bounds.py writes it: exact counts of the device code)
PEAK_TMAC_PER_S = 34.9                    # measured: v_mad_u64_u32, 8 waves/SIMD (profiles/r01_microbench_valu.txt)
HBM_PEAK_GBS = 8000.0
DUMP_ROWS = 32768                         # --dump-outputs: at most this many GT values (x 384 bytes x float32 = 48 MiB)


def dump_outputs(out_dir, gt):
    """--dump-outputs: the last timed step's GT values, a fixed seeded sample of rows when the batch has more than DUMP_ROWS, as
    out_dir/pair_gt.npy (rows x 384, one float32 per byte of gnark's in-memory struct: exact) + out_dir/pair_gt_index.npy (float64)."""
    n = gt.shape[0]
    idx = np.arange(n) if n <= DUMP_ROWS else np.sort(np.random.default_rng(wl.SEED).choice(n, DUMP_ROWS, replace=False))
    rows = gt[torch.from_numpy(idx).to(gt.device)].cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "pair_gt.npy"), rows.astype(np.float32))
    np.save(os.path.join(out_dir, "pair_gt_index.npy"), idx.astype(np.float64))


def usable_cpus():
    """CPUs this process may run on: the affinity mask, cut by the cgroup CPU quota when there is one (a GPU box hands a
    job a share of its cores; threads beyond the quota only add contention)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = max(1, min(n, int(int(quota) / int(period) + 0.5)))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(P, Q, gt_gpu, B):
    """Time the C restatement on a bounded sample of the same workload — on every thread count of a short ladder up to the
    usable CPUs, keeping the best (a quota the kernel does not publish shows up as a slower run at the larger counts) — then
    on one thread; bit-compare the GPU's outputs on the sample, and report the restatement's instrumented Fp-mul counts."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_lib
    oracle_lib.build()
    cap = usable_cpus()
    ladder = sorted({min(c, cap) for c in (8, 16, 32, 64, 128, 256, cap)})
    best = None
    tried = {}
    for threads in ladder:
        sample = min(B, 2048 * threads)                                      # ~2 s per rung
        Ps, Qs = P[:sample].cpu().numpy(), Q[:sample].cpu().numpy()
        oracle_lib.pair_batch(Ps[:threads], Qs[:threads], threads=threads)   # warm up the thread pool
        t0 = time.perf_counter()
        ref = oracle_lib.pair_batch(Ps, Qs, threads=threads)
        dt = time.perf_counter() - t0
        if not (ref == gt_gpu[:sample].cpu().numpy()).all():
            raise SystemExit("PARITY FAILURE: GPU pairings differ from the oracle on the cpu_baseline sample")
        tried[threads] = sample / dt
        if best is None or sample / dt > best[0]:
            best = (sample / dt, threads, sample)
        elif sample / dt < 0.8 * best[0]:
            break                                                            # past the quota: more threads only lose
    rate, threads, sample = best
    s1 = min(B, 8192)
    t0 = time.perf_counter()
    oracle_lib.pair_batch(P[:s1].cpu().numpy(), Q[:s1].cpu().numpy(), threads=1)
    dt1 = time.perf_counter() - t0
    what = "C restatement oracle/bn254_oracle.c (own port, NOT gnark-crypto: no Go toolchain on the box)"
    base = {"value": rate, "unit": "pairings/s", "cores": threads, "kind": "port",
            "sample": "%d pairs of the same synthetic batch, %s, OpenMP x%d (best of the thread counts %s; %d CPUs visible, %d usable); "
                      "GPU output bit-compared on every sample" % (sample, what, threads, sorted(tried), os.cpu_count() or 0, cap),
            "rate_by_threads": tried}
    one = {"value": s1 / dt1, "unit": "pairings/s", "cores": 1, "kind": "port", "sample": "%d pairs, one thread" % s1}
    try:
        counts = oracle_lib.fp_mul_counts()
    except Exception as exc:                                                # noqa: BLE001
        counts = {"error": repr(exc)}
    return base, one, counts


def main():
    em = os.path.join(ROOT, "profiles", "executed_mads.json")
    if os.path.exists(em):
        EXECUTED_MAD.update(json.load(open(em)).get("mads_per_unit", {}))
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=1 << 20, help="pairs per GPU per step (metric: 2^20)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write a fixed sample of the last timed step's GT values to DIR (rank 0)")
    ap.add_argument("--full", action="store_true", help="also the oracle check, per-kernel roofline, scalar-mult rates, extras, "
                                                         "config legs, PCIe / latency / CPU baselines (trimmed by the --no-* options)")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the extras and config legs")
    ap.add_argument("--no-configs", action="store_true", help="with --full: skip the BASELINE config 2-4 legs")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the CPU baseline (profiling runs)")
    ap.add_argument("--no-scalar-mul", action="store_true", help="with --full: skip the G1/G2 scalar-mult half of the metric (roofline.scalar_mul)")
    ap.add_argument("--config-scale", type=int, default=1, help="divide the config-leg sizes by this (quick runs; 1 = BASELINE sizes)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    use_dist = "RANK" in os.environ                      # launched by torch.distributed.run (any world size)
    # Rehearsal of the N > 1 control flow on a ONE-GPU box (GPBC_BENCH_REHEARSAL=1): every rank uses device 0, torch.distributed
    # runs on gloo and the library's RCCL communicator is skipped (RCCL refuses two ranks on one device), so the legs that need
    # the all-gather report an error entry.  Never a measurement: the line says so in config.rehearsal.
    # GPBC_BENCH_REHEARSAL=stub: the same, but WITH the library communicator — over tests/stub_rccl's librccl.so.1 (a test double that
    # rendezvouses the ranks' processes in shared memory), which must be on LD_LIBRARY_PATH: gpbc_comm_init_rank with N > 1 ranks and the
    # all-gather legs run for real, only the transport is not RCCL.
    rehearsal = use_dist and os.environ.get("GPBC_BENCH_REHEARSAL") in ("1", "stub")
    rehearsal_stub = rehearsal and os.environ.get("GPBC_BENCH_REHEARSAL") == "stub"
    if rehearsal:
        local_rank = 0
    if use_dist:
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        # RCCL prints its version banner on stdout when the communicator comes up: keep stdout for the ONE JSON line
        sys.stdout.flush()
        saved_stdout = os.dup(1)
        os.dup2(2, 1)
        try:
            if rehearsal:
                dist.init_process_group(backend="gloo")
            else:
                dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
            dist.barrier()
            torch.cuda.synchronize()
        finally:
            sys.stdout.flush()
            os.dup2(saved_stdout, 1)
            os.close(saved_stdout)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    from gopairingbasedcryptography_amd import _build, _lib, afp25, bn254, bsw07, sharding
    if rank == 0:
        _build.build_library()
    if use_dist:
        dist.barrier()
    bn254.init(local_rank)
    lib = _lib.load()
    comm_error = "rehearsal on one GPU: library communicator skipped" if (rehearsal and not rehearsal_stub) else None
    if use_dist and (not rehearsal or rehearsal_stub):
        # the library's own RCCL communicator over the same ranks (the all-gather of partial sums / GT rows)
        sys.stdout.flush()
        saved_stdout = os.dup(1)
        os.dup2(2, 1)
        try:
            sharding.init_library_comm(bn254)
        except Exception as exc:                                            # noqa: BLE001
            comm_error = repr(exc)
        finally:
            sys.stdout.flush()
            os.dup2(saved_stdout, 1)
            os.close(saved_stdout)

    def barrier():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(d):
        if use_dist:
            tm = torch.tensor([d], dtype=torch.float64, device=dev)
            dist.all_reduce(tm, op=dist.ReduceOp.MAX)
            d = float(tm.item())
        return d

    def all_ranks_true(flag):
        if use_dist:
            t = torch.tensor([1 if flag else 0], dtype=torch.int32, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            flag = bool(t.item())
        return bool(flag)

    B = args.batch
    # ---- synthetic inputs, generated by the engine's own scalar-mul kernels (timed as the secondary metric)
    g1, g2 = bn254.generators()
    g1d, g2d = torch.from_numpy(g1).to(dev), torch.from_numpy(g2).to(dev)
    kP = torch.from_numpy(wl.bench_scalars("P", rank * B, B).copy()).to(dev).reshape(B, 32)
    kQ = torch.from_numpy(wl.bench_scalars("Q", rank * B, B).copy()).to(dev).reshape(B, 32)
    P = bn254.g1_scalar_mul(g1d, kP)
    Q = bn254.g2_scalar_mul(g2d, kQ)
    torch.cuda.synchronize()
    f = torch.empty((B, 384), dtype=torch.uint8, device=dev)
    gt = torch.empty((B, 384), dtype=torch.uint8, device=dev)

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pP, pQ, pf, pgt = (ctypes.c_void_p(t.data_ptr()) for t in (P, Q, f, gt))
    nB = ctypes.c_size_t(B)

    def step():
        _lib.check(lib.gpbc_miller_loop_dev(pP, pQ, nB, pf, stream))
        _lib.check(lib.gpbc_final_exp_dev(pf, nB, pgt, stream))

    for _ in range(args.warmup):
        step()
    barrier()
    if args.full:
        _lib.check(lib.gpbc_profile_begin(stream))       # HIP events around every kernel of the timed steps, on their stream
    t0 = time.perf_counter()
    for s in range(args.steps):
        step()
    barrier()
    dt = max_over_ranks(time.perf_counter() - t0)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, gt)

    value = world * B * args.steps / dt
    result = {
        "metric": "BN254 pairings/s at batch 2^20 per GPU (+ G1/G2 scalar-mults/s at the same batch in roofline.scalar_mul)",
        "value": value, "unit": "pairings/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "int64", "data": "synthetic",
        "config": {"workload": "configs[1]: batch of %d independent bn254.Pair on random (G1,G2) points per GPU" % B,
                   "batch_per_gpu": B, "sharding": "independent index ranges per rank, no data-path collective",
                   "arithmetic": "254-bit Montgomery integers as 9 signed 29-bit limbs (int32), 32x32+64-bit MACs into int64 columns"},
    }
    if rehearsal:
        result["config"]["rehearsal"] = ("NOT A MEASUREMENT: %d ranks share one GPU (GPBC_BENCH_REHEARSAL), torch.distributed on gloo, " % world) + \
            ("library communicator over the rccl TEST DOUBLE of tests/stub_rccl" if rehearsal_stub else "no library communicator")

    def finish():
        if rank == 0:
            print(json.dumps(result))
        if use_dist:
            dist.barrier()
            try:
                bn254.comm_destroy()
            except Exception:                             # noqa: BLE001
                pass
            dist.destroy_process_group()

    if not args.full:
        return finish()
    names = ctypes.create_string_buffer(32 * 16)
    ms = (ctypes.c_double * 16)()
    cnt = (ctypes.c_int * 16)()
    nk = ctypes.c_int(0)
    _lib.check(lib.gpbc_profile_end(names, ms, cnt, 16, ctypes.byref(nk)))
    kern = {}
    for i in range(nk.value):
        nm = names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode()
        kern[nm] = {"ms_per_step": ms[i] / args.steps, "launches_per_step": cnt[i] / args.steps, "ms_per_launch": ms[i] / cnt[i]}
    # the roofline's denominator and the shader clock, measured in this process right after the timed steps (rank 0's device)
    probe = (ctypes.c_double * 4)()
    _lib.check(lib.gpbc_valu_probe(probe))
    peak_now, clock_hz = probe[0] / 1e12, probe[1]
    n_simd = 4 * torch.cuda.get_device_properties(dev).multi_processor_count
    # small --batch values take the pipelined or the latency kernel instead of the lines/accumulate pair: count whichever ran
    miller_ms = sum(v["ms_per_step"] for k, v in kern.items() if k in ("k_miller_lines", "k_miller_accumulate", "k_miller_pipelined", "k_miller_wide")) or float("nan")
    fexp_ms = kern.get("k_final_exp", {}).get("ms_per_step", float("nan"))

    # ---- every rank checks a sample of its own outputs against the oracle (the parity claim of the workload string)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_lib
    oracle_lib.build()
    si = np.r_[0:48, B // 2:B // 2 + 8, B - 8:B] if B >= 128 else np.arange(B)
    sample_ok = bool((oracle_lib.pair_batch(P[si].cpu().numpy(), Q[si].cpu().numpy(), threads=min(16, usable_cpus())) == gt[si].cpu().numpy()).all())
    if not all_ranks_true(sample_ok):
        raise SystemExit("PARITY FAILURE: rank %d: GPU pairings differ from the oracle on its sample" % rank if not sample_ok
                         else "PARITY FAILURE on another rank")
    result["config"]["workload"] += ("; every rank bit-compares %d of its outputs with the oracle (in-repo restatement: parity with "
                                     "gnark-crypto itself is unpinned, tests/test_gnark_vectors.py)" % len(si))
    # ---- roofline, VALU integer-MAC bound: the single kernel with the largest time per step
    frac = lambda fpmul, t_ms: fpmul * MAC_PER_FP_MUL * B / (t_ms * 1e-3) / 1e12 / PEAK_TMAC_PER_S
    # VALU instructions per wave of the same kernels from the last committed PMC pass (tools/pmc_run.sh -> profiles/pmc_counters.json):
    # NOT measured by this run — rocprofv3 counters need their own passes — but independent of the box's clock
    pmc = {}
    pp = os.path.join(ROOT, "profiles", "pmc_counters.json")
    if os.path.exists(pp):
        pmc = json.load(open(pp))
    for k, v in kern.items():
        if k in NOMINAL_FP_MUL:
            v["nominal_fp_mul"] = NOMINAL_FP_MUL[k]
            v["frac"] = frac(NOMINAL_FP_MUL[k], v["ms_per_step"])
            v["frac_same_run_peak"] = v["frac"] * PEAK_TMAC_PER_S / peak_now
            # clock-normalised: SIMD cycles the chip spent per pairing in this kernel (wall time x measured shader clock x SIMDs / batch)
            v["simd_cycles_per_pairing"] = v["ms_per_step"] * 1e-3 * clock_hz * n_simd / B
            if k in pmc.get("kernels", {}):
                v["valu_instr_per_wave_from_profiles"] = pmc["kernels"][k].get("valu_instr_per_wave")
    dom = max((k for k in kern if k in NOMINAL_FP_MUL), key=lambda k: kern[k]["ms_per_step"])
    launches = kern[dom]["launches_per_step"]
    achieved = NOMINAL_FP_MUL[dom] * MAC_PER_FP_MUL * (B / launches) / (kern[dom]["ms_per_launch"] * 1e-3) / 1e12
    algo_bytes = B * (64 + 128 + 384)
    traffic, per_kernel_traffic = None, {}
    tp = os.path.join(ROOT, "profiles", "pmc_traffic.json")          # written by tools/pmc_run.sh (separate --pmc passes)
    if os.path.exists(tp):
        tj = json.load(open(tp))
        for k in NOMINAL_FP_MUL:
            t = tj.get(k)
            if t:   # FETCH_SIZE is doubled per MI355X_MICROARCH.md (gfx950 counts 128-B requests as 64 B); KB -> bytes; per launch, times launches per step
                per_launch = (2 * t["fetch_kb"] + t["write_kb"]) * 1024.0
                per_kernel_traffic[k] = per_launch * (B / t["batch"])
        if len(per_kernel_traffic) == len(NOMINAL_FP_MUL):
            traffic = sum(per_kernel_traffic.values())
    def executed(unit, t_ms):
        """MADs the device code actually issues (profiles/executed_mads.json, counted by the interval harness) against the same-run peak:
        the share of the VALU's MAD rate spent on limb products, where `frac` prices SURVEY's nominal 136 MACs per Fp-mul"""
        m = EXECUTED_MAD.get(unit)
        return {"executed_mad_per_pairing": m, "executed_mad_frac_of_same_run_peak": m * B / (t_ms * 1e-3) / 1e12 / peak_now} if m else {}
    result["roofline"] = {
        "bound": "valu", "kernel": dom, "achieved": achieved, "peak": PEAK_TMAC_PER_S, "unit": "TMAC/s",
        "frac": achieved / PEAK_TMAC_PER_S,
        "peak_same_run": peak_now, "frac_same_run": achieved / peak_now,
        "probe": {"what": "gpbc_valu_probe: dependency-free v_mad_u64_u32 at 8 waves/SIMD, run in this process after the timed steps",
                  "tmac_per_s": peak_now, "shader_clock_GHz": clock_hz / 1e9, "simd_cycles_per_wave_instr": probe[2], "ms": probe[3]},
        "pmc_source": (pmc.get("source", "profiles/pmc_counters.json") + " — counters are from that committed rocprofv3 run, NOT from this run") if pmc else None,
        "kernel_ms_per_launch": kern[dom]["ms_per_launch"], "kernel_launches_per_step": launches, "pairs_per_launch": B / launches,
        "traffic": traffic, "traffic_unit": "HBM bytes per step, all kernels (PMC FETCH_SIZE x2 + WRITE_SIZE); from profiles/pmc_traffic.json (a committed rocprofv3 --pmc run), NOT measured by this run",
        "traffic_per_kernel": per_kernel_traffic or None, "algorithmic_bytes": algo_bytes,
        "traffic_over_algorithmic": (traffic / algo_bytes) if traffic else None,
        "kernels": kern,
        "stages": {"miller_loop (k_miller_lines + k_miller_accumulate)": {"ms": miller_ms, "nominal_fp_mul": FP_MUL_MILLER, "frac": frac(FP_MUL_MILLER, miller_ms),
                                                                           **executed("miller_loop", miller_ms)},
                   "k_final_exp": {"ms": fexp_ms, "nominal_fp_mul": FP_MUL_FINAL_EXP, "frac": frac(FP_MUL_FINAL_EXP, fexp_ms), **executed("final_exp", fexp_ms)}},
        "whole_pairing_frac": frac(FP_MUL_MILLER + FP_MUL_FINAL_EXP, miller_ms + fexp_ms),
        "hbm_GBs_algorithmic": algo_bytes / ((miller_ms + fexp_ms) * 1e-3) / 1e9, "hbm_peak_GBs": HBM_PEAK_GBS,
        "note": "integer carry-chain work: bound is VALU v_mad_i64_i32 issue, not HBM/MFMA (SURVEY.md §8d); peak = measured "
                "dependency-free v_mad_u64_u32 rate (profiles/r01_microbench_valu.txt); algorithmic MACs = nominal Fp-mul x 136; "
                "kernel times from HIP events on the launch stream around every launch of the timed steps",
    }
    sec = {}
    # ---- the other half of the metric: G1 / G2 scalar multiplications at the same batch (bases P_i / Q_i, scalars k("s", i)), HBM
    # resident, whole-job rate; the kernels' own time from the same HIP-event bracket as the pairing kernels
    ks = None
    if not args.no_scalar_mul:
        ks = torch.from_numpy(wl.bench_scalars("s", rank * B, B).copy()).to(dev).reshape(B, 32)
        smul = {}
        REPS = 2
        for name, fn, base, nominal in (("g1", bn254.g1_scalar_mul, P, FP_MUL_G1), ("g2", bn254.g2_scalar_mul, Q, FP_MUL_G2)):
            out = torch.empty_like(base)
            fn(base, ks, out=out)                       # untimed warm-up pass
            barrier()
            _lib.check(lib.gpbc_profile_begin(stream))
            t1 = time.perf_counter()
            for _ in range(REPS):
                fn(base, ks, out=out)
            barrier()
            d = max_over_ranks((time.perf_counter() - t1) / REPS)
            _lib.check(lib.gpbc_profile_end(names, ms, cnt, 16, ctypes.byref(nk)))
            kname = "k_%s_scalar_mul" % name
            k_ms, k_launches = None, None
            for i in range(nk.value):
                if names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode() == kname:
                    k_ms, k_launches = ms[i] / REPS, cnt[i] / REPS
            # the nominal count is SURVEY's (2 500 / 7 500 Fp-mul x 136); what the kernel EXECUTES is counted by the interval harness
            # (tools/bounds_check.cpp runs the device code on the host and counts its limb products): MADs per unit
            ex = EXECUTED_MAD.get(name)
            e = {"per_s": world * B / d, "unit": "%s scalar-mults/s, whole job, 254-bit scalars, one base per scalar" % name.upper(), "ms_per_batch": 1e3 * d,
                 "kernel": kname, "kernel_ms_per_batch": k_ms, "kernel_launches_per_batch": k_launches,
                 "nominal_fp_mul": nominal, "frac": nominal * MAC_PER_FP_MUL * B / d / 1e12 / PEAK_TMAC_PER_S,
                 "frac_same_run_peak": nominal * MAC_PER_FP_MUL * B / d / 1e12 / peak_now,
                 "kernel_frac": (nominal * MAC_PER_FP_MUL * B / (k_ms * 1e-3) / 1e12 / PEAK_TMAC_PER_S) if k_ms else None,
                 "simd_cycles_per_unit": (k_ms * 1e-3 * clock_hz * n_simd / B) if k_ms else None,
                 "executed_mad_per_unit": ex, "executed_mad_frac_of_same_run_peak": (ex * B / d / 1e12 / peak_now) if ex else None,
                 "valu_instr_per_wave_from_profiles": pmc.get("kernels", {}).get(kname, {}).get("valu_instr_per_wave")}
            smul[name] = e
            sec[name + "_scalar_mults_per_s"] = e["per_s"]
            sec[name + "_frac_of_valu_peak"] = e["frac"]
        result["roofline"]["scalar_mul"] = smul
    if not args.no_secondary:
        if ks is None:
            ks = torch.from_numpy(wl.bench_scalars("s", rank * B, B).copy()).to(dev).reshape(B, 32)

        # The remaining lines (wire formats, hash to curve, fixed-base tables, GT.Exp) are per-GPU rates of independent
        # kernels: measured on the single-GPU run only, and never allowed to take the headline JSON line down with them.
        def extras():
            def rate(fn, *a, **kw):
                fn(*a, **kw)
                barrier()
                t1 = time.perf_counter()
                fn(*a, **kw)
                barrier()
                return world * B / max_over_ranks(time.perf_counter() - t1)
            nw = min(B, 1 << 18)                              # the G2 subgroup check makes G2 decoding the slow one
            Pw, Qw, gw = P[:nw].contiguous(), Q[:nw].contiguous(), gt[:nw].contiguous()
            wire = {"batch": nw}
            for name, X, m, u in (("g1", Pw, bn254.g1_marshal, bn254.g1_unmarshal), ("g2", Qw, bn254.g2_marshal, bn254.g2_unmarshal)):
                comp, raw = m(X, compressed=True), m(X)
                wire[name + "_marshal_per_s"] = rate(m, X) * nw / B
                wire[name + "_compress_per_s"] = rate(m, X, compressed=True) * nw / B
                wire[name + "_unmarshal_raw_per_s"] = rate(u, raw, elem_bytes=raw.shape[1]) * nw / B
                wire[name + "_unmarshal_compressed_per_s"] = rate(u, comp, elem_bytes=comp.shape[1]) * nw / B
            wire["gt_marshal_per_s"] = rate(bn254.gt_marshal, gw) * nw / B
            wire["gt_unmarshal_per_s"] = rate(bn254.gt_unmarshal, bn254.gt_marshal(gw)) * nw / B
            sec["wire"] = wire
            uf = torch.from_numpy(wl.bench_scalars("h2c", rank * nw * 4, nw * 4).copy()).to(dev).reshape(-1, 32)   # values < r < p: valid fp.Elements
            sec["g1_map_to_curve_per_s"] = rate(bn254.map_to_g1, uf[:2 * nw].reshape(nw, 64).contiguous()) * nw / B
            sec["g2_map_to_curve_per_s"] = rate(bn254.map_to_g2, uf.reshape(nw, 128).contiguous()) * nw / B
            # whole hash to curve of 32-byte messages resident in HBM: SHA-256 expand_message_xmd + reduction + map, one message per lane
            hmsg = uf[:nw].reshape(-1).contiguous()
            hoff = (torch.arange(nw + 1, dtype=torch.int64, device=dev) * 32).contiguous()
            from gopairingbasedcryptography_amd import hash_to as _h2
            sec["g1_hash_to_curve_per_s"] = rate(lambda m: bn254.hash_to_g1(m, _h2.DST_BYTES_G1, msg_off=hoff), hmsg) * nw / B
            sec["g2_hash_to_curve_per_s"] = rate(lambda m: bn254.hash_to_g2(m, _h2.DST_BYTES_G2, msg_off=hoff), hmsg) * nw / B
            sec["hash_to_field_per_s"] = rate(lambda m: bn254.hash_to_field(m, _h2.DST_BYTES_G1, 2, msg_off=hoff), hmsg) * nw / B
            fb = bn254.FixedBase(g1d)
            sec["g1_fixed_base_mults_per_s"] = rate(fb.mul, ks)
            fb.close()
            nsrs, nmsm = 256, min(B // 256, 1024)
            fbs = bn254.FixedBase(P[:nsrs].contiguous())
            sec["g1_msm256_terms_per_s"] = rate(fbs.msm, ks[:nsrs * nmsm].contiguous()) * (nsrs * nmsm) / B
            fbs.close()
            # variable-base multi-scalar multiplication (bucket method): sum_i [s_i] P_i over the whole batch, full-width scalars
            sec["g1_msm_variable_base_terms_per_s"] = rate(bn254.g1_scalar_mul_sum, P, ks)
            sec["g2_msm_variable_base_terms_per_s"] = rate(bn254.g2_scalar_mul_sum, Q, ks)
            ne = min(B, 1 << 16)                              # GT.Exp by full-size exponents
            sec["gt_exp_per_s"] = rate(bn254.gt_exp, gt[:ne].contiguous(), ks[:ne].contiguous()) * ne / B
        if world == 1:
            try:
                extras()
            except Exception as exc:                      # noqa: BLE001
                sec["extras_error"] = repr(exc)

        # ---- BASELINE configs 2-4 at their stated sizes: totals are fixed (strong scaling over the ranks), every leg is checked
        def timed(fn):
            barrier()
            t1 = time.perf_counter()
            out = fn()
            barrier()
            return out, max_over_ranks(time.perf_counter() - t1)

        def guarded(setup, run):
            """A leg = rank-local setup (workload generation: the part that can fail on one rank alone) + a run with
            collectives.  The ranks agree that every setup succeeded before any of them enters the run, so a failure on one
            rank becomes an error entry on all of them instead of a hang in the next collective."""
            try:
                st, err = setup(), None
            except Exception as exc:                      # noqa: BLE001
                st, err = None, repr(exc)
            if not all_ranks_true(err is None):
                return {"error": err or "setup failed on another rank"}
            return run(st)

        def setup_aggregate():
            n_total = (1 << 20) // args.config_scale
            lo, hi = sharding.shard_range(n_total, rank, world)
            return n_total, wl.aggregate(bn254, hi - lo, dev, start=lo)

        def run_aggregate(st):
            n_total, inst = st
            # B = sum rho_i sigma_i over ALL ranks (untimed here; timed in the second figure)
            Bsum = bn254.g2_scalar_mul_sum(inst["sigma"], inst["rho"])
            def literal():                                    # "2^20 G1 scalar-mults + 2 pairings" (BASELINE configs[2])
                A = bn254.g1_scalar_mul_sum(inst["pk"], inst["rho"])          # + the 64 B-per-rank all-gather inside the library
                return wl.aggregate_check(bn254, A.cpu().numpy(), Bsum.cpu().numpy(), inst["H"], inst["g1"])
            literal()
            ok, t_lit = timed(literal)
            def full():
                A = bn254.g1_scalar_mul_sum(inst["pk"], inst["rho"])
                Bs = bn254.g2_scalar_mul_sum(inst["sigma"], inst["rho"])
                return wl.aggregate_check(bn254, A.cpu().numpy(), Bs.cpu().numpy(), inst["H"], inst["g1"])
            ok2, t_full = timed(full)
            forged = inst["sigma"].clone()
            if rank == 0:
                forged[1] = forged[0]
            Bf = bn254.g2_scalar_mul_sum(forged, inst["rho"])
            A = bn254.g1_scalar_mul_sum(inst["pk"], inst["rho"])
            rejected = not wl.aggregate_check(bn254, A.cpu().numpy(), Bf.cpu().numpy(), inst["H"], inst["g1"])
            return {"workload": "configs[2]: BLS aggregate verification of %d signatures on one message point, random linear "
                                "combination with 128-bit scalars" % n_total, "signatures": n_total, "scaling": "strong",
                    "signatures_per_s": n_total / t_lit, "ms": 1e3 * t_lit,
                    "timed": "sum rho_i pk_i over %d public keys (bucket multi-scalar multiplication: the result of that many G1 scalar-mults + their sum%s) + the 2-pairing check"
                             % (n_total, " + RCCL all-gather of the partial sums inside the library" if world > 1 else ""),
                    "with_g2_sums_signatures_per_s": n_total / t_full, "with_g2_sums_ms": 1e3 * t_full,
                    "accepts": all_ranks_true(ok and ok2), "rejects_forged": all_ranks_true(rejected),
                    "collective": ("library RCCL all-gather, %d ranks" % bn254.comm_ranks()) if world > 1 else None}

        def setup_bsw07(kind):
            n_total = (1 << 16) // args.config_scale
            lo, hi = sharding.shard_range(n_total, rank, world)
            inst = wl.bsw07_instance(bn254, kind, hi - lo, dev, start=lo)
            plan = bsw07.decrypt_plan(inst["tree"], inst["attrs"])
            folded = bsw07.fold_key(bn254, plan, inst["dj"], inst["dj_prime"])      # once per (key, policy), untimed
            return kind, n_total, inst, folded

        def run_bsw07(st):
            kind, n_total, inst, folded = st
            run = lambda: bsw07.decrypt_batch_arrays(bn254, folded, inst["D"], inst["c_tilde"], inst["c"], inst["cy"], inst["cy_prime"])
            run()
            out, t = timed(run)
            pairs = n_total * inst["pairs_per_ct"]
            return {"workload": "configs[3]: cpabe/bsw07 Decrypt, %s policy over 256 attributes, %d ciphertexts x %d pairs "
                                "(fixed-Q multi-pairing, Lagrange coefficients folded into the key)" % (kind, n_total, inst["pairs_per_ct"]),
                    "ciphertexts": n_total, "scaling": "strong", "ciphertexts_per_s": n_total / t, "pairs_per_s": pairs / t, "ms": 1e3 * t,
                    "all_messages_recovered": all_ranks_true(bool((out == inst["msgs"]).all()))}

        def setup_afp25():
            n_total, Bsz = (1 << 18) // args.config_scale, 256
            per = (n_total // Bsz // world) * Bsz                                   # whole batches per rank
            return per * world, Bsz, per, wl.afp25_instance(bn254, Bsz, per, dev, start=rank * per)

        def run_afp25(st):
            n_total, Bsz, per, inst = st
            gathered = [None]
            def run():
                out = afp25.decrypt_batch_arrays(bn254, inst["D"], inst["pi"], inst["sk"], inst["C1"], inst["C2"])
                if world > 1:                                                      # all-gather of the GT masks (BASELINE configs[4])
                    gathered[0] = bn254.allgather(out.reshape(-1))
                return out
            run()
            out, t = timed(run)
            ok = bool((out == inst["msgs"]).all())
            if world > 1:
                ok = ok and bool((gathered[0][rank].reshape(per, 384) == out).all())
            return {"workload": "configs[4]: bibe/afp25_bibe batch decryption of %d identities in batches of %d "
                                "(3-pair multi-pairing + GT.Div per item%s)" % (n_total, Bsz, ", RCCL all-gather of the GT masks inside the library" if world > 1 else ""),
                    "items": n_total, "scaling": "strong", "items_per_s": n_total / t, "pairs_per_s": 3 * n_total / t, "ms": 1e3 * t,
                    "all_messages_recovered": all_ranks_true(ok),
                    "collective": ("library RCCL all-gather of %d x 384 B per rank, %d ranks" % (per, bn254.comm_ranks())) if world > 1 else None}

        if not args.no_configs:
            cfg = {}
            if world > 1 and comm_error:
                cfg["comm_error"] = comm_error
            for key, setup, run in (("aggregate_verify_2^20", setup_aggregate, run_aggregate),
                                    ("bsw07_256of256_2^16", lambda: setup_bsw07("256of256"), run_bsw07),
                                    ("bsw07_16x16_2^16", lambda: setup_bsw07("16x16"), run_bsw07), ("afp25_2^18", setup_afp25, run_afp25)):
                try:
                    cfg[key] = guarded(setup, run)
                except Exception as exc:                  # noqa: BLE001
                    cfg[key] = {"error": repr(exc)}
                torch.cuda.empty_cache()
            sec["configs"] = cfg
        result["secondary"] = sec
    # ---- PCIe-inclusive rate and CPU baseline (rank 0, single-GPU run only)
    if rank == 0 and world == 1 and not args.no_cpu:
        try:
            Ph, Qh = P.cpu().numpy(), Q.cpu().numpy()
            gh = np.zeros((B, 384), dtype=np.uint8)                       # the caller's result buffer, pages already touched
            bn254.pair_batch(Ph, Qh, out=gh)                              # first call: stream / workspace creation
            t1 = time.perf_counter()
            bn254.pair_batch(Ph, Qh, out=gh)
            d = time.perf_counter() - t1
            result["value_pcie_inclusive"] = {"value": B / d, "unit": "pairings/s", "identical_to_hbm_resident_run": bool((gh == gt.cpu().numpy()).all()),
                                              "what": "gpbc_pair_batch on pageable host buffers: hipMalloc + 192 B/pair up + kernels + 384 B/pair down; "
                                                      "chunks of 131072 pairs alternate on two streams, a helper thread drains results on a third"}
            del Qh, gh
            kh = wl.bench_scalars("s", rank * B, B)
            oh = np.zeros((B, 64), dtype=np.uint8)                        # result buffer with its pages touched, as above
            bn254.g1_scalar_mul(Ph, kh, out=oh)                           # first call: per-stream table workspaces
            best = None
            for _ in range(2):
                t1 = time.perf_counter()
                bn254.g1_scalar_mul(Ph, kh, out=oh)
                d = time.perf_counter() - t1
                best = d if best is None or d < best else best
            result["value_pcie_inclusive"]["g1_scalar_mults_per_s"] = B / best
            del Ph, kh, oh
        except Exception as exc:                          # noqa: BLE001
            result["value_pcie_inclusive"] = {"error": repr(exc)}
        # latency of small host-pointer calls (what the reference's one-pairing-at-a-time call sites would see through the shim)
        try:
            lat = {}
            Ps, Qs = P[:4096].cpu().numpy(), Q[:4096].cpu().numpy()
            for m in (1, 2, 64, 4096):
                bn254.pair_batch(Ps[:m], Qs[:m])
                t1 = time.perf_counter()
                for _ in range(3):
                    bn254.pair_batch(Ps[:m], Qs[:m])
                lat["pair_batch_%d" % m] = 1e3 * (time.perf_counter() - t1) / 3
            bn254.pairing_check(Ps[:2], Qs[:2])
            t1 = time.perf_counter()
            for _ in range(3):
                bn254.pairing_check(Ps[:2], Qs[:2])
            lat["pairing_check_2_pairs"] = 1e3 * (time.perf_counter() - t1) / 3
            ksm = wl.bench_scalars("s", 0, 1)
            bn254.g1_scalar_mul(Ps[:1], ksm)
            t1 = time.perf_counter()
            for _ in range(3):
                bn254.g1_scalar_mul(Ps[:1], ksm)
            lat["g1_scalar_mul_1"] = 1e3 * (time.perf_counter() - t1) / 3
            # one BSW07-sized product (513 pairs, one final exponentiation) and one GT.Exp: the reference makes both one call at a time
            seg513 = np.array([0, 513], dtype=np.uint64)
            g513 = bn254.multi_pair(Ps[:513], Qs[:513], seg513)
            t1 = time.perf_counter()
            for _ in range(3):
                bn254.multi_pair(Ps[:513], Qs[:513], seg513)
            lat["multi_pair_1x513"] = 1e3 * (time.perf_counter() - t1) / 3
            gt1 = gt[:1].cpu().numpy()
            e1 = bn254.gt_exp(gt1, ksm)
            t1 = time.perf_counter()
            for _ in range(3):
                bn254.gt_exp(gt1, ksm)
            lat["gt_exp_1"] = 1e3 * (time.perf_counter() - t1) / 3
            # the same single calls on ONE host core through the C restatement (the cpu_baseline's port, bit-compared)
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import oracle_lib
            oracle_lib.build()
            cpu = {}
            for name, fn, want in (("pair_batch_1", lambda: oracle_lib.pair_batch(Ps[:1], Qs[:1], threads=1), gt[:1].cpu().numpy()),
                                   ("pairing_check_2_pairs", lambda: oracle_lib.multi_pair(Ps[:2], Qs[:2], np.array([0, 2], dtype=np.uint64), threads=1), None),
                                   ("multi_pair_1x513", lambda: oracle_lib.multi_pair(Ps[:513], Qs[:513], seg513, threads=1), g513),
                                   ("gt_exp_1", lambda: oracle_lib.gt_exp(gt1, ksm, threads=1), e1)):
                got = fn()
                reps = 1 if name == "multi_pair_1x513" else 5
                t1 = time.perf_counter()
                for _ in range(reps):
                    fn()
                cpu[name] = 1e3 * (time.perf_counter() - t1) / reps
                if want is not None and not (np.asarray(got).reshape(-1) == np.asarray(want).reshape(-1)).all():
                    raise SystemExit("PARITY FAILURE: single call %s differs from the oracle" % name)
            lat["one_host_core_port"] = cpu
            result["call_latency_ms"] = lat
        except Exception as exc:                          # noqa: BLE001
            result["call_latency_ms"] = {"error": repr(exc)}
        base, one, counts = cpu_baseline(P, Q, gt, B)
        result["cpu_baseline"], result["cpu_baseline_1core"], result["actual_fp_mul"] = base, one, counts
        # ---- the reference's call shape under concurrency: T OS threads looping one-element calls through the C ABI (native harness:
        # Python threads would measure the interpreter lock); a child process on the same device, this one idle meanwhile
        try:
            import subprocess
            exe = os.path.join(ROOT, "gopairingbasedcryptography_amd", "gpbc_concurrent_calls")
            cc = subprocess.run([exe, "--device", str(local_rank), "--seconds", "1", "--threads", "1,8,64"], capture_output=True, text=True, timeout=300)
            if cc.returncode != 0:
                raise RuntimeError("gpbc_concurrent_calls exit %d: %s" % (cc.returncode, (cc.stderr or cc.stdout)[-400:]))
            calls = json.loads(cc.stdout.strip().splitlines()[-1])
            if calls.get("mismatches"):
                raise SystemExit("PARITY FAILURE: concurrent single calls returned wrong bytes")
            result["concurrent_calls"] = calls
            base["concurrent_calls"] = {
                "what": "GPU: calls/s of T OS threads looping one-element gpbc_pair_batch / gpbc_pairing_check (2 pairs) / gpbc_g1_scalar_mul_batch "
                        "(tools/concurrent_calls.cpp, results compared); port: the C restatement's pairings/s on 1 and on %d threads" % base["cores"],
                "gpu_calls_per_s": {op: {t: v["calls_per_s"] for t, v in calls[op].items()} for op in ("pair_batch_1", "pairing_check_2_pairs", "g1_scalar_mul_1")},
                "port_pairings_per_s": {"1": one["value"], str(base["cores"]): base["value"]}}
        except SystemExit:
            raise
        except Exception as exc:                          # noqa: BLE001
            result["concurrent_calls"] = {"error": repr(exc)}
    finish()


if __name__ == "__main__":
    main()
