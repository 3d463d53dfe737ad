"""Child process of tests/test_small_calls_gpu.py: one phase of concurrent small host-pointer calls through the combiner
(csrc/gpbc_core.hip: small_call), every answer held against the oracle.

    python tests/small_calls_child.py PHASE [PHASE ...]

Runs in a process of its own because a thread asleep inside the C library cannot be cancelled: a lost wake-up must end at the parent's
time limit as a failed test.  Every expectation of a phase is computed BEFORE its first thread starts (oracle_lib / bn254_py; the
openers and the cap phase besides against ONE single-threaded call of more than 2 048 pairs, which takes the bulk route and other
kernels).  One JSON line per phase on stdout: the labels of the calls whose status or bytes were wrong, the statuses that were not
GPBC_OK, and the deltas of gpbc_small_call_stats.  After a phase with a wrong answer nothing more is started on the device.

Staging: the crowd's threads wait at a barrier; four openers per device slot each make one pair_batch of 2 048 pairs (a full batch of its
own, so each holds one of the slot's four lanes); the main thread releases the barrier once `batches` has risen by the number of
openers.  The crowd then queues behind busy lanes and the next leader takes it whole."""
import ctypes
import hashlib
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]

import numpy as np  # noqa: E402

import bn254_py as o  # noqa: E402
import oracle_lib as ol  # noqa: E402

CAP, OPENERS, CROWD, THREADS, OT = 2048, 4, 60, 64, 8            # OT: oracle threads (a constant: nothing here is sized by the machine)
OK, INVALID_ARG, INTERNAL, RAISED = 0, -1, -6, -99
R = o.R
EDGE_SCALARS = [0, R - 1, R, (1 << 256) - 1]
ONE = np.frombuffer(o.gt_to_bytes(o.F12_ONE), dtype=np.uint8)
G1 = np.frombuffer(o.g1_to_bytes(o.G1_GEN), dtype=np.uint8)
G2 = np.frombuffer(o.g2_to_bytes(o.G2_GEN), dtype=np.uint8)
FILL = 0xA5                                                       # what every output buffer holds before its call

L = None            # the loaded library (set in main)
bn254 = None
_drawn = 0          # points handed out so far: every call of a process gets points of its own


def vp(a):
    return None if a is None else a.ctypes.data


def rows32(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32).copy()


def scal(tag, n):
    """n distinct scalars below r, as rows (bench_scalar of the call's own label)"""
    return rows32(o.bench_scalar(tag, i) for i in range(n))


def pts(n):
    """n G1 and n G2 points nobody else in this process has: [s]G1, [t]G2 by the oracle"""
    global _drawn
    a = rows32(o.bench_scalar("small-calls/P", _drawn + i) for i in range(n))
    b = rows32(o.bench_scalar("small-calls/Q", _drawn + i) for i in range(n))
    _drawn += n
    return ol.g1_scalar_mul(G1, a, threads=OT), ol.g2_scalar_mul(G2, b, threads=OT)


def gts(n):
    return ol.pair_batch(*pts(n), threads=OT)


def out_rows(n, w):
    return np.full((n, w), FILL, dtype=np.uint8)


class Call:
    def __init__(self, label, fn, want, want_rc=OK):
        self.label, self.fn, self.want, self.want_rc = label, fn, want, want_rc
        self.rc, self.got, self.samples = None, None, None

    def run(self):
        try:
            self.rc, self.got = self.fn()
        except Exception as e:                                    # (the wrapper forms raise: the text goes into the report)
            self.rc, self.got = RAISED, [np.frombuffer(repr(e).encode()[:200], dtype=np.uint8)]

    def wrong(self):
        if self.rc != self.want_rc or len(self.got) != len(self.want):
            return True
        if any(g.shape != np.asarray(w).shape or not (g == w).all() for g, w in zip(self.got, self.want)):
            return True
        return self.samples is not None and not (self.got[0][self.samples[0]] == self.samples[1]).all()


# ------------------------------------------------------------------------------------------------ the ten combined kinds
def c_pair_batch(label, n, inf_p=(), inf_q=(), points=None, want=None):
    P, Q = points if points is not None else pts(n)
    for i in inf_p:
        P[i] = 0
    for i in inf_q:
        Q[i] = 0
    if want is None:
        want = ol.pair_batch(P, Q, threads=OT)

    def fn():
        out = out_rows(n, 384)
        return L.gpbc_pair_batch(vp(P), vp(Q), n, vp(out)), [out]
    return Call(label, fn, [want])


def c_multi_pair(label, seg, inf_p=(), inf_q=()):
    seg = np.array(seg, dtype=np.uint64)
    n, k = int(seg[-1]), len(seg) - 1
    P, Q = pts(n)
    for i in inf_p:
        P[i] = 0
    for i in inf_q:
        Q[i] = 0
    want = ol.multi_pair(P, Q, seg, threads=OT)

    def fn():
        out = out_rows(k, 384)
        return L.gpbc_multi_pair(vp(P), vp(Q), vp(seg), k, vp(out)), [out]
    return Call(label, fn, [want])


def c_pairing_check(label, pattern):
    """one segment per letter: T = e(P,Q) e(-P,Q) (true), F = e(P,Q)^2 (false), E = an empty segment (true)"""
    Ps, Qs, seg = [], [], [0]
    for ch in pattern:
        if ch != "E":
            P, Q = pts(1)
            Ps += [P[0], bn254.g1_neg(P[0]) if ch == "T" else P[0]]
            Qs += [Q[0], Q[0]]
        seg.append(len(Ps))
    P, Q, seg = np.array(Ps, dtype=np.uint8), np.array(Qs, dtype=np.uint8), np.array(seg, dtype=np.uint64)
    k = len(pattern)
    want = (ol.multi_pair(P, Q, seg, threads=OT) == ONE).all(axis=1).astype(np.uint8)
    assert want.tolist() == [0 if ch == "F" else 1 for ch in pattern], (label, want)          # the oracle itself agrees with the algebra

    def fn():
        ok = np.full(k, FILL, dtype=np.uint8)
        return L.gpbc_pairing_check(vp(P), vp(Q), vp(seg), k, vp(ok)), [ok]
    return Call(label, fn, [want])


def pairs_mix(label, idx, big=False):
    """the ragged mix of the pairs phases: neighbours differ in length, in table and in the flag they expect"""
    if big:
        return c_multi_pair(label + ":multi[0,300]", [0, 300])
    m = idx % 9
    if m == 0:
        return c_pair_batch(label + ":pairs1", 1)
    if m == 1:
        return c_pair_batch(label + ":pairs3,P[1]=inf", 3, inf_p=(1,))
    if m == 2:
        return c_pair_batch(label + ":pairs17,Q[16]=inf", 17, inf_q=(16,))
    if m == 3:
        return c_multi_pair(label + ":multi[0,0,2,2,5]", [0, 0, 2, 2, 5])
    if m == 4:
        return c_multi_pair(label + ":multi[0,4,4],P[0]=inf,Q[3]=inf", [0, 4, 4], inf_p=(0,), inf_q=(3,))
    if m == 5:
        return c_multi_pair(label + ":multi[0,1]", [0, 1])
    if m == 6:
        return c_pairing_check(label + ":check-true", "T")
    if m == 7:
        return c_pairing_check(label + ":check-false", "F")
    return c_pairing_check(label + ":check[T,E,F,T]", "TEFT")


def c_scalar_mul(label, g2, n, shared, first=None, last=None, inf_base=None):
    P, Q = pts(1 if shared else n)
    bases, w = (Q, 128) if g2 else (P, 64)
    k = scal(label, n)
    if first is not None:
        k[0] = rows32([first])[0]
    if last is not None:
        k[-1] = rows32([last])[0]
    if inf_base is not None:
        bases[inf_base] = 0
    nbase = len(bases)
    want = (ol.g2_scalar_mul if g2 else ol.g1_scalar_mul)(bases, k, threads=OT)
    entry = L.gpbc_g2_scalar_mul_batch if g2 else L.gpbc_g1_scalar_mul_batch

    def fn():
        out = out_rows(n, w)
        return entry(vp(bases), nbase, vp(k), n, vp(out)), [out]
    return Call(label, fn, [want])


def mul_mix(label, idx):
    g2, n = bool(idx & 1), (1, 2, 5, 64)[(idx >> 1) & 3]
    shared = bool((idx >> 3) & 1) and n > 1
    e = EDGE_SCALARS[(idx >> 4) & 3]
    first, last = (e, None) if (idx >> 6) & 1 else (None, e)
    inf = None
    if idx % 5 == 0:
        inf = 0 if shared or (idx % 10) else n - 1              # the one shared base, or the first / last base of the call
    name = "%s:%s n=%d %s %s=%s%s" % (label, "g2mul" if g2 else "g1mul", n, "one-base" if shared else "base-per-row",
                                      "k[0]" if first is not None else "k[-1]", ("0", "r-1", "r", "2^256-1")[(idx >> 4) & 3],
                                      "" if inf is None else " base[%d]=inf" % inf)
    return c_scalar_mul(name, g2, n, shared, first, last, inf)


def c_gt(label, op, n, one_a=(), one_b=(), k_first=None, k_last=None):
    a = gts(n)
    for i in one_a:
        a[i] = ONE
    if op == "exp":
        b = scal(label, n)
        if k_first is not None:
            b[0] = rows32([k_first])[0]
        if k_last is not None:
            b[-1] = rows32([k_last])[0]
        want, entry = ol.gt_exp(a, b, threads=OT), L.gpbc_gt_exp_batch
    elif op == "inv":
        b, want, entry = None, ol.gt_inverse(a), None
    else:
        b = gts(n)
        for i in one_b:
            b[i] = ONE
        want, entry = (ol.gt_mul(a, b), L.gpbc_gt_mul_batch) if op == "mul" else (ol.gt_div(a, b), L.gpbc_gt_div_batch)

    def fn():
        out = out_rows(n, 384)
        if op == "inv":
            return L.gpbc_gt_inverse_batch(vp(a), n, vp(out)), [out]
        return entry(vp(a), vp(b), n, vp(out)), [out]
    return Call(label, fn, [want])


def gt_mix(label, idx):
    op, n = ("exp", "mul", "div", "inv")[idx & 3], (1, 3, 8)[(idx >> 2) % 3]
    v = idx >> 2
    one_a = (n - 1,) if v % 4 == 1 else ()
    one_b = (0,) if v % 4 == 2 else ()
    kf = 0 if v % 2 == 0 else None
    kl = (R, R + 5, (1 << 256) - 1)[v % 3] if v % 4 != 3 else 0
    name = "%s:gt-%s n=%d" % (label, op, n) + (" a[-1]=1" if one_a else "") + (" b[0]=1" if one_b and op in ("mul", "div") else "")
    if op == "exp":
        name += " k[0]=%s k[-1]=%s" % ("0" if kf == 0 else "rand", "0" if kl == 0 else ">=r")
    return c_gt(name, op, n, one_a, one_b, kf, kl)


def message(tag, length):
    return hashlib.shake_256(tag.encode()).digest(length) if length else b""


def c_hash(label, g2, msgs, dst, null_msgs=False, want_rc=OK):
    n, w = len(msgs), 128 if g2 else 64
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    data = None if null_msgs else np.frombuffer(b"".join(msgs) + b"\0", dtype=np.uint8).copy()        # (never an empty array)
    assert not null_msgs or int(off[-1]) == 0
    dbuf = np.frombuffer(dst, dtype=np.uint8).copy() if dst else None
    if want_rc == OK:
        enc = (lambda m: o.g2_to_bytes(o.hash_to_g2(m, dst))) if g2 else (lambda m: o.g1_to_bytes(o.hash_to_g1(m, dst)))
        want = np.frombuffer(b"".join(enc(m) for m in msgs), dtype=np.uint8).reshape(n, w)
    else:
        want = out_rows(n, w)                                     # a refused call writes nothing
    entry = L.gpbc_hash_to_g2 if g2 else L.gpbc_hash_to_g1

    def fn():
        out = out_rows(n, w)
        return entry(vp(data), vp(off), n, vp(dbuf), len(dst), vp(out)), [out]
    return Call(label, fn, [want], want_rc)


DST_STEM = b"GPBC-V01-SMALL-CALLS-with-BN254G_XMD:SHA-256_SVDW_RO_"
DSTS = [DST_STEM + b"A", DST_STEM + b"B", DST_STEM + b"C", b"", bytes(range(1, 256))]
MSG_LENGTHS = [0, 1, 55, 56, 64, 1000]


def hash_mix(label, idx):
    d, g2, three = idx % 5, bool((idx // 5) & 1), bool((idx // 10) & 1)
    lens = [MSG_LENGTHS[(idx + 2 * j) % 6] for j in range(3 if three else 1)]
    name = "%s:hash-%s dst#%d lens=%s" % (label, "g2" if g2 else "g1", d, lens)
    return c_hash(name, g2, [message("%s/%d" % (name, j), n) for j, n in enumerate(lens)], DSTS[d])


class Tables:
    """two G1 tables (one base, three bases) and one G2 table alive at once; every table's own answer alone first"""
    def __init__(self):
        self.items = []
        for name, g2, nbase in (("g1x1", False, 1), ("g1x3", False, 3), ("g2x2", True, 2)):
            P, Q = pts(nbase)
            bases = Q if g2 else P
            self.items.append((name, g2, bases, bn254.FixedBase(bases, g2=g2)))

    def call(self, label, which, n_msm):
        name, g2, bases, fb = self.items[which]
        nb, w = len(bases), 128 if g2 else 64
        label = "%s:fixed-base %s n_msm=%d" % (label, name, n_msm)
        k = scal(label, n_msm * nb)
        mul, add = (ol.g2_scalar_mul, ol.g2_sum) if g2 else (ol.g1_scalar_mul, ol.g1_sum)
        want = np.array([add(mul(bases, k[i * nb:(i + 1) * nb], threads=OT)) for i in range(n_msm)], dtype=np.uint8)
        h = fb._h

        def fn():
            out = out_rows(n_msm, w)
            return L.gpbc_fixed_base_msm(h, vp(k), n_msm, vp(out)), [out]
        return Call(label, fn, [want])

    def close(self):
        for _, _, _, fb in self.items:
            fb.close()


# ------------------------------------------------------------------------------------------------ the uncombined lane users
def c_wrapped(label, call, want):
    def fn():
        got = call()
        return OK, [np.asarray(g) for g in (got if isinstance(got, tuple) else (got,))]
    return Call(label, fn, want)


def lane_mix(label, idx):
    m = idx % 6
    if m == 0:
        P, _ = pts(1)
        enc = np.frombuffer(o.g1_marshal(o.g1_from_bytes(P[0].tobytes())), dtype=np.uint8).reshape(1, 64)
        return c_wrapped(label + ":g1_marshal 1", lambda: bn254.g1_marshal(P), [enc])
    if m == 1:
        _, Q = pts(1)
        enc = np.frombuffer(o.g2_marshal(o.g2_from_bytes(Q[0].tobytes())), dtype=np.uint8).reshape(1, 128).copy()
        return c_wrapped(label + ":g2_unmarshal 1", lambda: bn254.g2_unmarshal(enc), [Q, np.ones(1, dtype=np.uint8)])
    if m == 2:
        a, b = pts(8)[0], pts(8)[0]
        want = np.array([ol.g1_sum(np.stack([a[i], b[i]])) for i in range(8)], dtype=np.uint8)
        return c_wrapped(label + ":g1_add 8", lambda: bn254.g1_add(a, b), [want])
    if m == 3:
        a, b = scal(label + "/a", 8), scal(label + "/b", 8)
        ints = lambda r: [int.from_bytes(x.tobytes(), "little") for x in r]
        want = rows32(x * y % R for x, y in zip(ints(a), ints(b)))
        return c_wrapped(label + ":fr_mul 8", lambda: bn254.fr_mul(a.reshape(-1), b.reshape(-1)).reshape(8, 32), [want])
    if m == 4:
        msgs = [message("%s/%d" % (label, j), n) for j, n in enumerate((3, 0, 200))]
        dst = DSTS[idx % 3]
        want = np.frombuffer(b"".join(o.fp_to_mont_bytes(u) for msg in msgs for u in o.hash_to_field_fp(msg, dst, 2)), dtype=np.uint8).reshape(3, 64)
        return c_wrapped(label + ":hash_to_field 3", lambda: bn254.hash_to_field(msgs, dst, 2), [want])
    x, k, seg = gts(16), scal(label, 16), [0, 7, 16]
    p = ol.gt_exp(x, k, threads=OT)
    want = []
    for lo, hi in zip(seg, seg[1:]):
        acc = p[lo:lo + 1]
        for i in range(lo + 1, hi):
            acc = ol.gt_mul(acc, p[i:i + 1])
        want.append(acc[0])
    return c_wrapped(label + ":gt_multi_exp 16 in [0,7,16]", lambda: bn254.gt_multi_exp(x, k.reshape(-1), seg), [np.array(want, dtype=np.uint8)])


# ------------------------------------------------------------------------------------------------ staging and the report
def stats():
    return bn254.small_call_stats()


def sample_rows(lo, hi, n):
    return lo + np.linspace(0, hi - lo - 1, n).astype(np.int64)


def make_openers(n_slots, mism, extra=0):
    """4 x 2 048 pairs per slot (and `extra` pairs for the caller) by ONE single-threaded call of more than 2 048 pairs, which takes the bulk
    route; 64 of every opener's pairs (128 of the extra ones) by the oracle as well.  Returns the opener calls and, of the extra pairs,
    (P, Q, bulk values, sample indices, oracle rows)."""
    n_open = OPENERS * n_slots
    n = n_open * CAP
    P, Q = pts(n + extra)
    before = stats()
    ref = bn254.pair_batch(P, Q)
    assert n > CAP and stats() == before                          # the reference did not come through the combiner
    idx = np.concatenate([sample_rows(i * CAP, (i + 1) * CAP, 64) for i in range(n_open)] + ([sample_rows(n, n + extra, 128)] if extra else []))
    rows = ol.pair_batch(P[idx], Q[idx], threads=OT)
    if not (ref[idx] == rows).all():
        mism.append("reference: the bulk route against the oracle")
    calls = []
    for i in range(n_open):
        lo, hi = i * CAP, (i + 1) * CAP
        c = c_pair_batch("opener%d:pairs2048" % i, CAP, points=(P[lo:hi].copy(), Q[lo:hi].copy()), want=ref[lo:hi])
        c.samples = (idx[64 * i:64 * (i + 1)] - lo, rows[64 * i:64 * (i + 1)])
        calls.append(c)
    return calls, (P[n:], Q[n:], ref[n:], idx[64 * n_open:] - n, rows[64 * n_open:])


def stage(crowd, openers, n_slots=1, knob=False):
    """crowd: one list of calls per thread.  Returns (staged, [batches, calls, largest_batch, failed_in_shared_batches]): deltas, but for
    largest_batch, a maximum since load — everything this process did before its first crowd was single-threaded (batches of one)."""
    s0 = stats()
    gate = threading.Barrier(len(crowd) + 1)

    def bind(slot):
        if n_slots > 1:
            assert L.gpbc_set_device(slot) == OK

    def member(t, calls):
        bind(t % n_slots)
        gate.wait()
        for c in calls:
            c.run()

    def opener(i, c):
        bind(i // OPENERS)
        c.run()
    ths = [threading.Thread(target=member, args=(t, calls)) for t, calls in enumerate(crowd)]
    for th in ths:
        th.start()
    while gate.n_waiting < len(crowd):
        time.sleep(0.0005)
    oth = [threading.Thread(target=opener, args=(i, c)) for i, c in enumerate(openers)]
    for th in oth:
        th.start()
    staged, give_up = True, time.time() + 20
    while stats()[0] - s0[0] < len(openers):
        if time.time() > give_up or not any(th.is_alive() for th in oth):
            staged = False
            break
        time.sleep(0.0002)
    if knob:
        time.sleep(0.002)                                         # every opener has read its table by now; its kernels run for far longer
        assert L.gpbc_debug_stale_table_once() == OK
    gate.wait()
    for th in ths + oth:
        th.join()
    s1 = stats()
    return staged, [s1[0] - s0[0], s1[1] - s0[1], s1[2], s1[3] - s0[3]]


def judge(calls, mism, statuses):
    for c in calls:
        if c.rc != OK:
            statuses[c.label] = c.rc
        if c.wrong():
            mism.append(c.label)


def crowd_of(threads, per_thread, make):
    return [[make("t%02d.%d" % (t, j), per_thread * t + j) for j in range(per_thread)] for t in range(threads)]


def phase_pairs(n_slots=1):
    mism, statuses = [], {}
    openers, _ = make_openers(n_slots, mism)
    crowd = crowd_of(CROWD, 2, lambda label, idx: pairs_mix(label, idx, big=idx == 51))
    staged, d = stage(crowd, openers, n_slots)
    judge(openers + [c for calls in crowd for c in calls], mism, statuses)
    return dict(mismatches=mism, statuses=statuses, staged=staged, stats=d, crowd=CROWD, crowd_calls=2 * CROWD)


def phase_cap():
    mism, statuses = [], {}
    sizes = [100] * 40 + [CAP, CAP + 1]
    openers, (P, Q, ref, idx, rows) = make_openers(1, mism, extra=sum(sizes))
    crowd, lo = [], 0
    for t, n in enumerate(sizes):
        c = c_pair_batch("t%02d.0:pairs%d" % (t, n), n, points=(P[lo:lo + n].copy(), Q[lo:lo + n].copy()), want=ref[lo:lo + n])
        pick = (idx >= lo) & (idx < lo + n)
        c.samples = (idx[pick] - lo, rows[pick])
        crowd.append([c])
        lo += n
    staged, d = stage(crowd, openers)
    judge(openers + [c for calls in crowd for c in calls], mism, statuses)
    # 2 049 pairs leave the combiner: 41 crowd calls are counted, and 4 000 + 2 048 units need three batches at least
    return dict(mismatches=mism, statuses=statuses, staged=staged, stats=d, crowd=len(sizes), crowd_calls=len(sizes) - 1)


def phase_generic(make, per_thread=2, threads=CROWD, extra=(), setup=None):
    mism, statuses = [], {}
    openers, _ = make_openers(1, mism)
    ctx = setup(mism) if setup else None
    crowd = crowd_of(threads, per_thread, (lambda label, idx: make(ctx, label, idx)) if setup else make)
    for t, c in extra:
        crowd[t].append(c() if ctx is None else c(ctx))
    staged, d = stage(crowd, openers)
    judge(openers + [c for calls in crowd for c in calls], mism, statuses)
    if ctx is not None:
        ctx.close()
    return dict(mismatches=mism, statuses=statuses, staged=staged, stats=d, crowd=threads, crowd_calls=sum(len(c) for c in crowd))


def phase_hash():
    extra = [
        (7, lambda: c_hash("t07.2:hash-g1 dst#0 three empty messages, NULL message pointer", False, [b"", b"", b""], DSTS[0], null_msgs=True)),
        (8, lambda: c_hash("t08.2:hash-g2 dst#4 three empty messages, NULL message pointer", True, [b"", b"", b""], DSTS[4], null_msgs=True)),
        # a tag of 256 bytes is refused by the library (as gnark's ExpandMsgXmd refuses it); it is never combined: the refusal comes from a
        # lane of its own, which must be free again afterwards
        (9, lambda: c_hash("t09.2:hash-g1 256-byte dst (refused)", False, [b"abc"], bytes(256), want_rc=INVALID_ARG)),
        (10, lambda: c_hash("t10.2:hash-g2 256-byte dst (refused)", True, [b"abc", b""], bytes(range(256)), want_rc=INVALID_ARG)),
    ]
    return phase_generic(hash_mix, extra=extra)


def tables_setup(mism):
    tb = Tables()
    # every table alone first, single-threaded, against the oracle (its later answers are held against the same oracle rows)
    for which in range(3):
        for n_msm in (1, 4):
            c = tb.call("alone", which, n_msm)
            c.run()
            if c.wrong():
                mism.append(c.label)
    return tb


def phase_fixed_base():
    return phase_generic(lambda tb, label, idx: tb.call(label, idx % 3, (1, 4)[(idx // 3) & 1]), setup=tables_setup)


def everything(tb, label, idx):
    t, j = idx // 4, idx % 4
    kind = (t + 5 * j) % 16                                       # sixteen kinds, rotated per thread
    v = idx // 16
    if kind == 0:
        return pairs_mix(label, v)
    if kind in (1, 2):
        return c_scalar_mul("%s:%s n=%d" % (label, "g2mul" if kind == 2 else "g1mul", (1, 5)[v & 1]), kind == 2, (1, 5)[v & 1], bool(v & 2) and bool(v & 1))
    if kind in (3, 4, 5, 6):
        return c_gt("%s:gt-%s" % (label, ("exp", "mul", "div", "inv")[kind - 3]), ("exp", "mul", "div", "inv")[kind - 3], (1, 3)[v & 1])
    if kind in (7, 8):
        lens = [MSG_LENGTHS[(v + 2 * i) % 6] for i in range((1, 3)[v & 1])]
        name = "%s:hash-%s dst#%d lens=%s" % (label, "g2" if kind == 8 else "g1", v % 2, lens)
        return c_hash(name, kind == 8, [message("%s/%d" % (name, i), n) for i, n in enumerate(lens)], DSTS[v % 2])
    if kind == 9:
        return tb.call(label, v % 3, (1, 4)[v & 1])
    return lane_mix(label, kind - 10)


def phase_everything():
    return phase_generic(everything, per_thread=4, threads=THREADS, setup=tables_setup)


def phase_fail_closed():
    os.environ["GPBC_TEST_KNOBS"] = "1"                           # this phase alone; read by the library when the knob is armed
    mism, statuses, rounds, total = [], {}, [], [0, 0, 0, 0]
    staged = True
    openers, _ = make_openers(1, mism)                            # (the same four in every round: run() overwrites their results)
    for r in range(6):
        crowd = crowd_of(CROWD, 1, lambda label, idx: pairs_mix("round%d.%s" % (r, label), idx + 7 * r, big=idx == 30 + r))
        ok, d = stage(crowd, openers, knob=True)
        staged = staged and ok
        total = [total[0] + d[0], total[1] + d[1], d[2], total[3] + d[3]]
        rounds.append(d)
        calls = openers + [c for cs in crowd for c in cs]
        failed = [c for c in calls if c.rc != OK]
        for c in failed:
            statuses[c.label if c.label.startswith("round") else "round%d.%s" % (r, c.label)] = c.rc
        if len(failed) != 1:
            mism.append("round%d: %d calls failed, exactly one must" % (r, len(failed)))
        for c in calls:
            if c in failed:
                # withheld: GPBC_ERR_INTERNAL and every GT value / flag of that call zero
                if c.rc != INTERNAL or any(g.any() for g in c.got):
                    mism.append(c.label + " (the failed call: status %d, outputs %s)" % (c.rc, "not zeroed" if any(g.any() for g in c.got) else "zeroed"))
            elif c.wrong():
                mism.append(c.label)
        if mism:
            break
    return dict(mismatches=mism, statuses=statuses, staged=staged, stats=total, crowd=6 * CROWD, crowd_calls=6 * CROWD, rounds=len(rounds))


PHASES = {
    "pairs": phase_pairs,
    "cap": phase_cap,
    "scalar_mul": lambda: phase_generic(mul_mix),
    "gt": lambda: phase_generic(gt_mix),
    "hash": phase_hash,
    "fixed_base": phase_fixed_base,
    "everything": phase_everything,
    "two_slots": lambda: phase_pairs(n_slots=2),
    "fail_closed": phase_fail_closed,
}


def main(argv):
    global L, bn254
    names = argv[1:]
    if not names or any(n not in PHASES for n in names):
        print("usage: small_calls_child.py PHASE...   phases: " + " ".join(PHASES), file=sys.stderr)
        return 2
    from gopairingbasedcryptography_amd import _lib, bn254 as _bn254
    bn254 = _bn254
    L = _lib.load()
    ol.build()
    two = "two_slots" in names
    if two and len(names) > 1:
        print("two_slots binds its own device list: run it alone", file=sys.stderr)
        return 2
    bn254.init([0, 0] if two else 0)
    bad = False
    for name in names:
        t0 = time.time()
        rep = PHASES[name]()
        rep.update(phase=name, seconds=round(time.time() - t0, 2))
        rep["stats"] = dict(zip(("batches", "calls", "largest_batch", "failed_in_shared_batches"), rep["stats"]))
        print(json.dumps(rep), flush=True)
        if rep["mismatches"]:
            bad = True
            break                                                 # nothing more on the device after a wrong answer
    bn254.shutdown()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
