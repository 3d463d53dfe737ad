"""The small-call combiner (csrc/gpbc_core.hip: small_call, and the batch runners small_rows_run / small_pairs_run / small_hash_run /
small_mul_run / small_gt_run / small_fixed_base_run) under many threads: calls of different sizes, keys and tables that SHARE launches,
every caller's bytes against the oracle.  A wrong offset in a runner is not a crash, it is caller A receiving caller B's answer; the
device entries never combine and tests/cpp/test_threads.cpp makes calls of one element only, so this is the suite's view of that code.

Each phase runs tests/small_calls_child.py in a fresh child process, one at a time (a thread asleep inside the C library cannot be
cancelled: a lost wake-up ends at the child's time limit as a failed test).  The child stages every phase behind four openers that hold
the four call lanes (its docstring), computes every expectation before a thread starts, and reports the mismatching calls by label, the
statuses and the deltas of gpbc_small_call_stats; the assertions are here.

The counter conditions are conditions, not measurements: a phase whose calls did not share launches has tested nothing and fails.
    largest_batch >= 2   and   calls - batches >= half the crowd's threads
(`batches` counts the openers' four batches of one call each, which add nothing to calls - batches.)

Wall time of each child on an MI355X, measured once (process start, library load and the oracle's expectations included; the phase
itself, expectations included, took 0.6 .. 2.3 s of it), in seconds:
    pairs 3.0   cap 2.9   scalar_mul 2.7   gt 3.4   hash 2.9   fixed_base 2.6   everything 3.5   two_slots 3.3   fail_closed 4.2
The time limit of a child is ten times that and at least 60 s, which is 60 s for every phase.
"""
import json
import os
import subprocess
import sys
import time

import pytest

from conftest import ROOT

CHILD = os.path.join(ROOT, "tests", "small_calls_child.py")
# phase -> wall seconds of its child, measured on the MI355X (the docstring above)
MEASURED = {"pairs": 3.0, "cap": 2.9, "scalar_mul": 2.7, "gt": 3.4, "hash": 2.9, "fixed_base": 2.6, "everything": 3.5, "two_slots": 3.3,
            "fail_closed": 4.2}


def run_phase(phase):
    limit = max(60.0, 10 * MEASURED[phase])
    env = {k: v for k, v in os.environ.items() if k != "GPBC_TEST_KNOBS"}          # the child sets it itself, for the failure phase alone
    t0 = time.time()
    r = subprocess.run([sys.executable, CHILD, phase], capture_output=True, text=True, timeout=limit, env=env)
    wall = time.time() - t0
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    print("small-calls child %s: %.1f s wall, exit %d\n%s" % (phase, wall, r.returncode, "\n".join(lines)))
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    rep = json.loads(lines[-1])
    assert rep["phase"] == phase
    assert rep["mismatches"] == [], (rep["mismatches"][:20], rep["statuses"])
    assert r.returncode == 0, r.stderr[-4000:]
    assert rep["staged"], "the openers never held the four lanes"
    return rep


def shared_launches(rep, more_batches=0):
    """the phase was not vacuous: its calls rode in each other's launches"""
    s = rep["stats"]
    assert s["largest_batch"] >= 2, s
    assert s["calls"] - s["batches"] >= rep["crowd"] // 2, (s, rep["crowd"])
    assert s["batches"] >= 4 + more_batches, s
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("phase", ["pairs", "scalar_mul", "gt", "fixed_base", "two_slots"])
def test_calls_that_share_a_launch_get_their_own_slices(phase):
    """ragged pair_batch / multi_pair / pairing_check (empty segments, infinity in either slot, one 300-pair segment, neighbours with
    opposite flags); G1 / G2 scalar multiplication with one base and a base per row, edge scalars first and last; GT exp / mul / div /
    inverse; fixed-base sums over three tables alive at once; the pairs mix again on both slots of a {0, 0} device list"""
    rep = run_phase(phase)
    s = shared_launches(rep)
    assert rep["statuses"] == {} and s["failed_in_shared_batches"] == 0
    # every crowd call was served by the combiner (and the openers' four, or eight on two slots)
    assert s["calls"] == rep["crowd_calls"] + (8 if phase == "two_slots" else 4)


@pytest.mark.gpu
def test_cap_and_route_boundary():
    """40 calls of 100 pairs, one of exactly 2 048 and one of 2 049: a request that does not fit the batch waits for the next leader, and
    2 049 pairs leave the combiner for the bulk route while it is busy"""
    rep = run_phase("cap")
    s = shared_launches(rep, more_batches=2)
    assert rep["statuses"] == {} and s["calls"] == 4 + 41          # the call of 2 049 is not a small call


@pytest.mark.gpu
def test_hash_calls_share_a_launch_only_under_one_tag():
    """five tags (three that differ in the last byte, the empty one, 255 bytes), messages of 0 .. 1 000 bytes, calls of empty messages with a
    null message pointer; a tag of 256 bytes is refused from a lane of its own"""
    rep = run_phase("hash")
    s = shared_launches(rep)
    assert sorted(rep["statuses"].values()) == [-1, -1] and all("256-byte dst" in k for k in rep["statuses"])
    assert s["failed_in_shared_batches"] == 0 and s["calls"] == 4 + rep["crowd_calls"] - 2


@pytest.mark.gpu
def test_every_kind_at_once_stays_live():
    """all ten combined kinds and six uncombined lane users from 64 threads, four calls each, kinds rotated per thread: every result is
    checked, and the child's time limit is what catches a lost wake-up"""
    rep = run_phase("everything")
    s = shared_launches(rep)
    assert rep["statuses"] == {} and s["failed_in_shared_batches"] == 0 and rep["crowd"] == 64 and rep["crowd_calls"] == 256
    assert s["calls"] == 4 + 160                                   # ten of the sixteen kinds go through the combiner


@pytest.mark.gpu
def test_fail_closed_call_by_call():
    """six rounds with the stale-table knob armed once the lanes are held: per round exactly one call (openers included) returns
    GPBC_ERR_INTERNAL with its outputs zeroed, every other call GPBC_OK with the oracle's bytes; over the rounds the failing call sat
    in a shared batch at least once, or the isolation was never exercised"""
    rep = run_phase("fail_closed")
    s = shared_launches(rep)
    assert rep["rounds"] == 6 and sorted(rep["statuses"].values()) == [-6] * 6, rep["statuses"]
    assert s["failed_in_shared_batches"] >= 1, s
