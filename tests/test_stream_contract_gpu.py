"""The stream contract of the device entries (include/gpbc_bn254.h, "The stream contract"; run with -m gpu): every kernel, copy and
memset of a *_dev call is enqueued on the caller's stream and on no other, the call reads its inputs behind the earlier work of that
stream, and it returns without waiting for the stream unless BLOCKING below names the line of code that makes it wait.

How a stream is gated.  On a side stream the argument tensors of a case hold a DECOY (valid inputs with another answer); then, all
on that stream: a device-side delay of bounded length (the gate), copies of the REAL inputs over the arguments, an event `filled`,
the entry, clones of its results, copies of the decoy back over the arguments.  A kernel that was launched on another stream, or a
host read of an input outside the stream's order, sees the decoy, because the gate is still closed when the call is made and the
decoy is back when a late kernel runs; the clones then differ from the host form's answer on the real inputs.  `filled.query()` right
after the call says whether the gate was still closed when the call returned: for an entry that is not in BLOCKING it must have
been.  Every case is run ungated first (twice: the first run grows the workspaces, the second is timed), and the gate is ten times
the slowest timed return of a non-blocking case of the same family, at least 20 ms and at most 250 ms.

The cases are the table of tests/test_host_device_forms_gpu.py at n = 5, the same entries at the sizes where they take another
kernel (SIZED below), and three chains of calls side by side on three streams.  What the entries compute is held against the oracle
elsewhere; pair_batch, the scalar multiplications, gt_exp and multi_pair are compared with it here as well."""
import contextlib
import math
import threading
import time

import numpy as np
import pytest

from test_host_device_forms_gpu import Offsets, arguments, cases, results

pytestmark = pytest.mark.gpu

# ---- entries that may make the host wait for the stream, each with the code that does it.  "C" rows are the list of
# include/gpbc_bn254.h; "Python" rows are wrappers of bn254.py over C entries that do not wait.  DESIGN.md "Stream contract" has both.
BLOCKING = {
    "hostseg": ("C", "gpbc_multi_pair_hostseg_dev (multi_pair: device points, host table)",
                "csrc/gpbc_pairing.hip multi_pair_core: hipMemcpyAsync(h_echo, dEcho, ...) then hipStreamSynchronize(st) before verify_echo"),
    "check": ("C", "gpbc_check_segments_dev (multi_pair and gt_multi_exp with a device table validate it first)",
              "csrc/gpbc_pairing.hip gpbc_check_segments_dev: hipStreamSynchronize(st) after the read-back of the flag; DevBuf's release drains the device"),
    "msm": ("C", "gpbc_g1_scalar_mul_sum_dev / gpbc_g2_scalar_mul_sum_dev from 16 384 terms on",
            "csrc/gpbc_msm.hip msm_run: 'read-back of the longest buckets', hipMemcpyAsync(pin, total, ...) || hipStreamSynchronize(st)"),
    "fixed_base": ("C", "gpbc_fixed_base_create_dev, and FixedBase() / FixedBase.msm / FixedBase.mul over it and over gpbc_fixed_base_msm_dev",
                   "csrc/gpbc_curve.hip gpbc_fixed_base_create_dev: hipMalloc of the table; bn254.FixedBase.__init__ and FixedBase.msm: "
                   "_current_stream().synchronize() (the bases / the workspace may be released on return)"),
    "put": ("Python", "a host value beside device buffers: gt_exp with host or Python exponents, gt_multi_exp / gt_prod with a host table or host "
                      "exponents, g1/g2_scalar_mul_base on a tensor (the generator)",
            "_buffers.put: torch.from_numpy(...).to(device) from pageable memory returns when the copy on the current stream is done"),
    "pairing_check": ("C", "gpbc_pairing_check (pairing_check, pairing_check_batch): host buffers only, no device form",
                      "bn254._pairs(host_only=True) refuses tensors; synchronous like every host-pointer entry"),
}
BLOCKS = {
    "multi_pair": "hostseg", "multi_pair whole": "hostseg", "multi_pair device table": "check",
    "g1_scalar_mul_base": "put", "g2_scalar_mul_base": "put",
    "g1 FixedBase.mul": "fixed_base", "g1 FixedBase.msm": "fixed_base", "g2 FixedBase.mul": "fixed_base", "g2 FixedBase.msm": "fixed_base",
    "gt_exp Python ints": "put", "gt_exp host exponents": "put",
    "gt_multi_exp": "put", "gt_multi_exp device table": "check", "gt_multi_exp host exponents": "put",
    "gt_multi_exp one list": "put", "gt_multi_exp one list, device table": "check",
    "gt_prod": "put", "gt_prod segments": "put",
    # SIZED
    "g1_scalar_mul_sum n=16500": "msm", "g2_scalar_mul_sum n=16500": "msm",
    "gt_multi_exp one segment of 5": "put", "gt_multi_exp one segment of 37": "put", "gt_prod one segment of 37": "put",
}
assert set(BLOCKS.values()) <= set(BLOCKING)

# A whole-array reduction gives the same answer on rolled rows, so its decoy also loses a row: the first row repeats the second.
REDUCES = ("_sum", "gt_prod", "multi_pair whole", "gt_multi_exp one segment")
# Symbols the gated cases need not reach (the assertion of test_every_device_symbol_is_reached): the two all-gather entries need a
# communicator, which one process on one device does not have.
EXEMPT = {"gpbc_allgather_dev": "needs a communicator (RCCL over two ranks)", "gpbc_allgather_all_dev": "needs a communicator over all bound devices"}
GATE_MIN_MS, GATE_MAX_MS = 20.0, 250.0


# ------------------------------------------------------------------------------------------------ the rig
class Rig:
    """the engine, at most three side streams, the gate, and what the families have found so far"""

    def __init__(self, eng):
        import torch
        self.eng, self.torch = eng, torch
        self.streams = [torch.cuda.Stream() for _ in range(3)]
        self.seen, self.found, self.numbers = set(), {}, {}
        torch.cuda.synchronize()
        if hasattr(torch.cuda, "_sleep"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(10 ** 5)                                            # (the first call pays the kernel's load)
            e0.record()
            torch.cuda._sleep(10 ** 7)
            e1.record()
            e1.synchronize()
            self.cycles_per_ms = 1e7 / e0.elapsed_time(e1)
            self.unit_ms = None
        else:                                                                     # a fixed chain of the engine's own final_exp calls on 2^16 values
            self.cycles_per_ms = None
            self.block = torch.zeros((1 << 16, 384), dtype=torch.uint8, device="cuda")
            eng.final_exp(self.block)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.final_exp(self.block)
            e1.record()
            e1.synchronize()
            self.unit_ms = e0.elapsed_time(e1)
        print("\nstream contract: %s" % ("%.0f sleep cycles per ms" % self.cycles_per_ms if self.cycles_per_ms else "one final_exp of 2^16 values = %.2f ms" % self.unit_ms))

    def gate(self, ms):
        """a device-side delay of about `ms` on the current stream, bounded by construction"""
        if self.cycles_per_ms:
            self.torch.cuda._sleep(int(ms * self.cycles_per_ms))
        else:
            for _ in range(int(math.ceil(ms / self.unit_ms))):
                self.eng.final_exp(self.block)


class Recorder:
    """the loaded library with every *_dev symbol that is called written down"""

    def __init__(self, lib, seen):
        self._lib, self._seen = lib, seen

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.endswith("_dev"):
            return fn

        def called(*args):
            self._seen.add(name)
            return fn(*args)
        return called


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


@pytest.fixture(scope="module")
def rig(eng):
    return Rig(eng)


# ------------------------------------------------------------------------------------------------ decoys
def decoy_of(label, a, turn=1):
    """one argument's decoy: its rows rolled by `turn` (a flat buffer of scalars of the Fr entries: by one scalar), an offset table with
    its inner entries one lower, message bytes inverted; an argument of one row, or one that is no buffer, stays"""
    if isinstance(a, Offsets):
        v = list(a.values)
        inner = [max(x - 1, 0) for x in v[1:-1]]
        return Offsets(v[:1] + inner + v[-1:])
    if not isinstance(a, np.ndarray):
        return a
    if label.startswith("hash_to") and a.ndim == 1:
        return a ^ np.uint8(0x5A)
    if a.ndim == 1:                                           # (one point, a flat list of scalars)
        return np.roll(a, 32) if label.startswith("fr_") and a.size > 32 else a.copy()
    d = np.roll(a, turn, axis=0)
    if any(word in label for word in REDUCES) and a.shape[0] > 2:
        d[0] = d[1]
    return d


def decoys(label, args):
    """The first array of a call is rolled by one row, the second by two, and so on: operands that mirror each other (g1_add of the
    points and the points reversed gives the same sum in every row) would give the same answer if both were rolled alike."""
    out, turn = [], 1
    for a in args:
        out.append(decoy_of(label, a, turn))
        if isinstance(a, np.ndarray) and a.ndim > 1 and a.shape[0] > 1:
            turn += 1
    return tuple(out)


def same_bytes(xs, ys):
    return len(xs) == len(ys) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(xs, ys))


def host_answer(fn, args):
    return [np.array(r, copy=True) for r in results(fn(*arguments(args, False)))]


def prepare(label, fn, args):
    """(expected results, decoy arguments, whether the decoy's answer differs)"""
    want = host_answer(fn, args)
    decoy = decoys(label, args)
    try:
        other = host_answer(fn, decoy)
    except ValueError:                                        # the rolled table is refused with this entry's other arguments (a shared exponent list): keep the table
        decoy = tuple(a if isinstance(a, Offsets) else d for a, d in zip(args, decoy))
        other = host_answer(fn, decoy)
    return want, decoy, other


# ------------------------------------------------------------------------------------------------ the gated procedure
ORACLE = {
    "pair_batch": lambda o, a: o.pair_batch(a[0], a[1], threads=4),
    "multi_pair": lambda o, a: o.multi_pair(a[0], a[1], a[2].values if isinstance(a[2], Offsets) else a[2], threads=4),
    "g1_scalar_mul": lambda o, a: o.g1_scalar_mul(a[0], a[1], threads=4),
    "g2_scalar_mul": lambda o, a: o.g2_scalar_mul(a[0], a[1], threads=4),
    "gt_exp": lambda o, a: o.gt_exp(a[0], a[1], threads=4),
}
ORACLE_LABELS = {"pair_batch": "pair_batch", "multi_pair": "multi_pair", "multi_pair whole": "multi_pair", "multi_pair device table": "multi_pair",
                 "g1_scalar_mul": "g1_scalar_mul", "g1_scalar_mul one base": "g1_scalar_mul", "g2_scalar_mul": "g2_scalar_mul",
                 "g2_scalar_mul one base": "g2_scalar_mul", "gt_exp": "gt_exp"}


def run_family(rig, family, case_list, oracle=None):
    """the gated procedure on every case; returns the list of what is wrong (strings) and records it under `family`"""
    if family in rig.found:
        return rig.found[family]
    from gopairingbasedcryptography_amd import _lib
    torch, s = rig.torch, rig.streams[0]
    wrong, work = [], []
    for label, fn, args, _ in case_list:
        want, decoy, other = prepare(label, fn, args)
        if same_bytes(want, other):
            wrong.append("%s: the decoy gives the same answer as the real inputs" % label)
        real_d, decoy_d = arguments(args, True), arguments(decoy, True)
        slots = [i for i, a in enumerate(real_d) if torch.is_tensor(a)]
        live = list(real_d)
        for i in slots:
            live[i] = decoy_d[i].clone()
        work.append((label, fn, args, want, other, real_d, decoy_d, slots, live))
    torch.cuda.synchronize()

    def one(item, gate_ms):
        label, fn, _, _, _, real_d, decoy_d, slots, live = item
        with torch.cuda.stream(s):
            if gate_ms:
                rig.gate(gate_ms)
            for i in slots:
                live[i].copy_(real_d[i], non_blocking=True)
            filled = torch.cuda.Event()
            filled.record(s)
            t0 = time.perf_counter()
            res = results(fn(*live))
            dt = (time.perf_counter() - t0) * 1e3
            closed = not filled.query()
            snaps = [r.clone() for r in res]
            for i in slots:
                live[i].copy_(decoy_d[i], non_blocking=True)
        s.synchronize()
        return dt, closed, snaps

    slowest = 0.0
    for timed in (False, True):                               # workspaces and the allocator's blocks are warm after the first pass
        for item in work:
            dt, _, _ = one(item, 0)
            if timed and item[0] not in BLOCKS:
                slowest = max(slowest, dt)
    gate_ms = min(max(10 * slowest, GATE_MIN_MS), GATE_MAX_MS)
    rig.numbers[family] = (slowest, gate_ms)
    print("\n%s: slowest non-blocking return %.3f ms, gate %.0f ms" % (family, slowest, gate_ms))
    real_lib = _lib._lib
    _lib._lib = Recorder(real_lib, rig.seen)
    try:
        for item in work:
            label, _, args, want, other = item[:5]
            dt, closed, snaps = one(item, gate_ms)
            got = [t.cpu().numpy() for t in snaps]
            print("  %-44s returned in %8.3f ms, gate %s%s" % (label, dt, "closed" if closed else "open", "  (may block: %s)" % BLOCKS[label] if label in BLOCKS else ""))
            if label not in BLOCKS and not closed:
                wrong.append("%s: returned after %.3f ms with the gate of %.0f ms already open: it waited for the stream, and BLOCKING does not say why" % (label, dt, gate_ms))
            if not same_bytes(want, got):
                wrong.append("%s: the gated result differs from the host form on the real inputs%s" % (label, " and equals the answer on the decoy" if same_bytes(other, got) else ""))
            if oracle is not None and label in ORACLE_LABELS:
                if not same_bytes([ORACLE[ORACLE_LABELS[label]](oracle, args)], [g.reshape(len(g), -1) for g in got]):
                    wrong.append("%s: the gated result differs from the oracle" % label)
    finally:
        _lib._lib = real_lib
    rig.found[family] = wrong
    return wrong


# ------------------------------------------------------------------------------------------------ 1. the table of the two forms, by family
FAMILIES = {
    "pairings": ("pair_batch", "multi_pair", "miller_loop", "final_exp"),
    "g1": ("g1",),
    "g2": ("g2",),
    "fr": ("fr_",),
    "gt": ("gt_",),
    "hash": ("map_to", "hash_to"),
}


def table_family(eng, family):
    return [c for c in cases(eng, 5) if c[0].startswith(FAMILIES[family])]


def test_the_families_cover_the_table(eng):
    labels = [c[0] for c in cases(eng, 5)]
    in_family = [label for f in FAMILIES for label in labels if label.startswith(FAMILIES[f])]
    assert sorted(in_family) == sorted(labels)
    assert {k for k in BLOCKS if " n=" not in k and "one segment of" not in k} <= set(labels)       # no stale row in the table of blocking entries


@pytest.mark.parametrize("family", list(FAMILIES))
def test_ordered_behind_the_stream(eng, rig, oracle, family):
    wrong = run_family(rig, family, table_family(eng, family), oracle)
    assert not wrong, "\n".join(wrong)


# ------------------------------------------------------------------------------------------------ 2. the sizes where an entry takes another route
def scalars(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


class Pool:
    """points made once with the engine's generator multiplications and shared by the sized cases and the chains"""

    def __init__(self, eng):
        self.P = eng.g1_scalar_mul_base(list(range(1, 33001)))
        self.Q = eng.g2_scalar_mul_base(list(range(1, 16386)))
        self.S = scalars(33000, 7)


@pytest.fixture(scope="module")
def pool(eng):
    return Pool(eng)


@contextlib.contextmanager
def chunk(pairs):
    """the pairs per shared-squaring chunk of the multi-pairings set for a while: multi_pair_fixed_q then takes the line-table route at
    a size of the latency route"""
    from gopairingbasedcryptography_amd import _lib
    _lib.check(_lib.load().gpbc_set_multi_pair_chunk(pairs))
    try:
        yield
    finally:
        _lib.load().gpbc_set_multi_pair_chunk(0)


def with_chunk(eng, pairs):
    def call(P, Q):
        with chunk(pairs):
            return eng.multi_pair_fixed_q(P, Q)
    return call


def sized(eng, pool, family):
    P, Q, S = pool.P, pool.Q, pool.S
    none = ()
    if family == "pairing sizes":             # latency form (5, in the table), pipelined launch, two-kernel form with the line workspace
        for n in (2049, 16385):
            yield "pair_batch n=%d" % n, eng.pair_batch, (P[:n].copy(), Q[:n].copy()), none
            yield "miller_loop n=%d" % n, eng.miller_loop, (P[:n].copy(), Q[:n].copy()), none
        yield "final_exp n=4097", eng.final_exp, (eng.miller_loop(P[:4097], Q[:4097]),), none
    if family == "scalar multiplication sizes":
        g1, g2 = eng.generators()
        for g, pts, gen in (("g1", P, g1), ("g2", Q, g2)):
            for n in (2049, 16385):
                yield "%s_scalar_mul n=%d" % (g, n), getattr(eng, g + "_scalar_mul"), (pts[:n].copy(), S[:n].copy()), none
            yield "%s_scalar_mul one base n=16385" % g, getattr(eng, g + "_scalar_mul"), (gen, S[:16385].copy()), none      # the transient table
            for n in (16, 16500):
                base = pts[:n] if len(pts) >= n else np.concatenate([pts, pts[:n - len(pts)]])
                yield "%s_scalar_mul_sum n=%d" % (g, n), getattr(eng, g + "_scalar_mul_sum"), (base.copy(), S[:n].copy()), none
    if family == "gt sizes":
        GT = eng.pair_batch(P[:4097], Q[:4097])
        yield "gt_exp n=4097", eng.gt_exp, (GT, S[:4097].copy()), none
        for n in (5, 37):                      # segred_pieces with GT_MEXP_SHAPE: one segment is cut, and its pieces folded, from 8 factors with exponents and 16 without
            yield "gt_multi_exp one segment of %d" % n, eng.gt_multi_exp, (GT[:n].copy(), S[:n].copy(), [0, n]), none
        yield "gt_prod one segment of 37", eng.gt_prod, (GT[:37].copy(),), none                                   # (5 factors: "gt_prod" of the table)
    if family == "fixed q sizes":
        yield "multi_pair_fixed_q 13 x 11", eng.multi_pair_fixed_q, (P[:143].copy(), Q[:11].copy()), none
        yield "multi_pair_fixed_q 70 x 3, chunk 24", with_chunk(eng, 24), (P[:210].copy(), Q[:70].copy()), none
    if family == "wire and hash sizes":
        for n in (2049, 16385):
            yield "g2_unmarshal compressed n=%d" % n, eng.g2_unmarshal, (eng.g2_marshal(Q[:n], True), 64), none
            data = np.frombuffer(b"".join(i.to_bytes(7, "little") for i in range(n)), dtype=np.uint8)
            yield "hash_to_g2 n=%d" % n, eng.hash_to_g2, (data, b"sizes", Offsets(list(range(0, 7 * n + 1, 7)))), none
    if family == "fr sizes":                   # 64 lanes per workgroup; an inversion lane holds 8 elements, a Lagrange lane 4 outputs
        k = 1031
        yield "fr_inverse n=1031", eng.fr_inverse, (S[:k].copy(),), none
        yield "fr_lagrange_basis n=1031", eng.fr_lagrange_basis, (S[:3 * k].reshape(-1, 32).copy(), 3), none
        roots = S[:2 * k].copy()
        yield "fr_poly_quotients n=1031", eng.fr_poly_quotients, (eng.fr_poly_from_roots(roots, 2).reshape(-1), roots, 2, 3), none
        matrix = eng.fr_to_bytes([1, 1, 0, eng.R_ORDER - 1, 1, 0]).copy()
        held = (np.arange(3 * k).reshape(k, 3) * 2654435761 >> 7 & 1).astype(np.uint8)
        held[::5] = (1, 1, 0)
        yield "fr_lsss_weights n=1031", eng.fr_lsss_weights, (np.tile(matrix, k), 3, 2, held), none


SIZED = ("pairing sizes", "scalar multiplication sizes", "gt sizes", "fixed q sizes", "wire and hash sizes", "fr sizes")


@pytest.mark.parametrize("family", SIZED)
def test_ordered_behind_the_stream_at_every_route(eng, rig, pool, family):
    wrong = run_family(rig, family, list(sized(eng, pool, family)))
    assert not wrong, "\n".join(wrong)


# ------------------------------------------------------------------------------------------------ 3. every device symbol
def test_every_device_symbol_is_reached(eng, rig, oracle):
    """the gated cases of the table at n = 5 call every gpbc_*_dev symbol of _lib.SIGNATURES but the two all-gather entries"""
    from gopairingbasedcryptography_amd import _lib
    wrong = []
    for family in FAMILIES:
        wrong += run_family(rig, family, table_family(eng, family), oracle)
    declared = {name for name in _lib.SIGNATURES if name.endswith("_dev")}
    assert set(EXEMPT) <= declared
    missing = sorted(declared - set(EXEMPT) - rig.seen)
    assert not missing, "no gated case calls %s" % ", ".join(missing)
    assert not wrong, "\n".join(wrong)


# ------------------------------------------------------------------------------------------------ 4. streams side by side
def chain_inputs(rig, pool, f):
    """the device inputs of the three chains at `f` times the first round's batch, every chain with points and scalars of its own"""
    torch = rig.torch
    P, Q, S = pool.P, pool.Q, pool.S
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n, k, t = 3000 * f, 3 * f, 16500 * f
    A = dict(P1=dev(P[:n]), Q1=dev(Q[:n]), S=dev(S[:n]), P2=dev(P[n:2 * n]), Q2=dev(Q[n:2 * n][::-1]))
    B = dict(P=dev(P[20000:20000 + 70 * k]), Q=dev(Q[12000:12070]), D=dev(rig.eng.pair_batch(P[:k], Q[:k])))
    C = dict(P=dev(P[25000:25000 + 70 * k]), Q=dev(Q[13000:13070]), Qs=dev(Q[6000:6000 + n]), S=dev(S[10000:10000 + n]), Pm=dev(P[:t]), Sm=dev(S[:t][::-1]))
    torch.cuda.synchronize()
    return A, B, C


def chains(eng, inputs):
    """every chain as a list of steps on a dict of its results"""
    A, B, C = inputs
    fixed_q = eng.multi_pair_fixed_q           # under chunk(24), the line-table route: B and C keep a line table in their stream's scratch between calls
    return [
        [lambda r: r.update(g=eng.pair_batch(A["P1"], A["Q1"])), lambda r: r.update(e=eng.gt_exp(r["g"], A["S"])),
         lambda r: r.update(h=eng.pair_batch(A["P2"], A["Q2"])), lambda r: r.update(m=eng.gt_mul(r["e"], r["h"]))],
        [lambda r: r.update(f=fixed_q(B["P"], B["Q"])), lambda r: r.update(d=eng.gt_div(r["f"], B["D"]))],
        [lambda r: r.update(f=fixed_q(C["P"], C["Q"])), lambda r: r.update(q=eng.g2_scalar_mul(C["Qs"], C["S"])),
         lambda r: r.update(s=eng.g2_sum(r["q"])), lambda r: r.update(t=eng.g1_scalar_mul_sum(C["Pm"], C["Sm"]))],
    ]


def to_host(states):
    return [{k: v.cpu().numpy().tobytes() for k, v in r.items()} for r in states]


def alone(rig, inputs):
    """every chain by itself on the default stream, synchronised after each call"""
    states = []
    for steps in chains(rig.eng, inputs):
        r = {}
        for step in steps:
            step(r)
            rig.torch.cuda.synchronize()
        states.append(r)
    return to_host(states)


def round_robin(rig, inputs, streams, release=False):
    """one host thread enqueues the chains a call at a time in turn; nothing synchronises until the end (but release_workspaces, which
    the round that asks for it calls once after the first call of every chain, with the rest still to come)"""
    torch = rig.torch
    todo = chains(rig.eng, inputs)
    states, at = [{} for _ in todo], 0
    while any(at < len(steps) for steps in todo):
        for steps, r, s in zip(todo, states, streams):
            if at < len(steps):
                with torch.cuda.stream(s):
                    steps[at](r)
        if release and at == 0:
            rig.eng.release_workspaces()
        at += 1
    for s in streams:
        s.synchronize()
    return to_host(states)


def threaded(rig, inputs, streams):
    """one Python thread per chain, each on the stream given for it (two chains may be given the same one)"""
    torch = rig.torch
    todo = chains(rig.eng, inputs)
    states, errors = [{} for _ in todo], []

    def run(steps, r, s):
        try:
            with torch.cuda.stream(s):
                for step in steps:
                    step(r)
        except Exception as e:                                # reported by the caller: an exception in a thread is otherwise lost
            errors.append(repr(e))

    threads = [threading.Thread(target=run, args=(steps, r, s)) for steps, r, s in zip(todo, states, streams)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a chain did not return within 120 s"
    assert not errors, "\n".join(errors)
    for s in set(streams):
        s.synchronize()
    return to_host(states)


def differences(got, want, what):
    return ["%s: chain %s, result %s differs from the chain run alone" % (what, "ABC"[c], k) for c, (g, w) in enumerate(zip(got, want)) for k in w if g.get(k) != w[k]]


@pytest.fixture(scope="module")
def rounds(rig, pool):
    """the inputs of the first round and of the round at twice the batch, and what the chains give alone"""
    out = {}
    with chunk(24):
        for f in (1, 2):
            inputs = chain_inputs(rig, pool, f)
            out[f] = (inputs, alone(rig, inputs))
    return out


def test_three_streams_side_by_side(rig, rounds):
    """a first round, a round at twice the batch (every stream's workspace regrows while the other two have work queued), and a round
    with a release_workspaces() from the enqueueing thread while work is still queued"""
    wrong = []
    with chunk(24):
        for what, f, release in (("first round", 1, False), ("round at twice the batch", 2, False), ("round with release_workspaces", 1, True)):
            wrong += differences(round_robin(rig, rounds[f][0], rig.streams, release), rounds[f][1], what)
    assert not wrong, "\n".join(wrong)


def test_one_thread_per_stream(rig, rounds):
    wrong = []
    with chunk(24):
        for what, f in (("first round", 1), ("round at twice the batch", 2)):
            wrong += differences(threaded(rig, rounds[f][0], rig.streams), rounds[f][1], what)
    assert not wrong, "\n".join(wrong)


def test_two_threads_share_one_stream(rig, rounds):
    """chains B and C, each with buffers of its own, from two threads on ONE stream (their line tables share that stream's scratch:
    the scratch lock keeps the enqueues of one call together), chain A beside them on another"""
    a, b = rig.streams[0], rig.streams[1]
    wrong = []
    with chunk(24):
        for what, f in (("first round", 1), ("round at twice the batch", 2)):
            wrong += differences(threaded(rig, rounds[f][0], [a, b, b]), rounds[f][1], what)
    assert not wrong, "\n".join(wrong)
