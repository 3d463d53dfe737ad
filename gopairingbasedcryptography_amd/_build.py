"""Compile libgpbc_bn254.so for gfx950 with hipcc (in-tree, next to this file).

Eleven translation units (csrc/gpbc_core.hip, gpbc_pairing.hip, gpbc_curve.hip, gpbc_wire.hip, gpbc_msm.hip, gpbc_group.hip, gpbc_fr.hip, gpbc_gtmexp.hip,
gpbc_gmsm.hip, gpbc_subset.hip, gpbc_hash.hip) are compiled in parallel and
linked into one shared library; every unit carries its own device code (no relocatable device code is needed: kernels are
launched from the unit that defines them).  A twelfth, csrc/gpbc_member.hip, is listed beside them (MEMBER_SOURCES), and a thirteenth,
csrc/gpbc_gtfixed.hip (GTFIXED_SOURCES), and a fourteenth, csrc/gpbc_openings.hip (OPENINGS_SOURCES)."""
import hashlib
import os
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libgpbc_bn254.so")
STAMP = os.path.join(HERE, "libgpbc_bn254.buildhash")
SOURCES = ["gpbc_core.hip", "gpbc_pairing.hip", "gpbc_curve.hip", "gpbc_wire.hip", "gpbc_msm.hip", "gpbc_group.hip", "gpbc_fr.hip", "gpbc_gtmexp.hip", "gpbc_gmsm.hip", "gpbc_subset.hip"]
# The eleventh unit, the entries of include/gpbc_bn254_hash.h.  A list of its own beside SOURCES, as its header and its signature table
# are beside theirs: tests/test_subset_sum.py holds SOURCES at the ten units above.  UNITS is what is compiled, scanned and hashed.
HASH_SOURCES = ["gpbc_hash.hip"]
UNITS = SOURCES + HASH_SOURCES
# The twelfth unit, the entries of include/gpbc_bn254_member.h, again in a list of its own: the tests that came with the earlier headers hold
# UNITS at the eleven above.  ALL_UNITS is what is compiled, scanned and hashed.  (Why the membership kernels are not in gpbc_pairing.hip and
# gpbc_wire.hip, beside the code they call: the head of csrc/gpbc_member.hip.)
MEMBER_SOURCES = ["gpbc_member.hip"]
ALL_UNITS = UNITS + MEMBER_SOURCES
# The thirteenth unit, the entries of include/gpbc_bn254_gtfixed.h, in a list of its own once more: tests/test_membership.py holds ALL_UNITS at
# the twelve above.  ALL_UNITS + GTFIXED_SOURCES is what is compiled, scanned and hashed.  (Why the kernels are not beside k_gt_exp in
# gpbc_pairing.hip: the head of csrc/gpbc_gtfixed.hip.)
GTFIXED_SOURCES = ["gpbc_gtfixed.hip"]
# The fourteenth unit, the entries of include/gpbc_bn254_openings.h, in a list of its own for the same reason: tests/test_gt_fixed_base.py holds
# the text ALL_UNITS + GTFIXED_SOURCES in the three functions below.  ALL_UNITS + GTFIXED_SOURCES + OPENINGS_SOURCES is what is compiled, scanned
# and hashed.  (Why the kernels are not beside fb_msm_lane in gpbc_curve.hip: the head of csrc/gpbc_openings.hip.)
OPENINGS_SOURCES = ["gpbc_openings.hip"]
HEADERS = ["gpbc_common.hpp", "fe29.hip.hpp", "tower29.hip.hpp", "tower29_pair.hip.hpp", "curve29.hip.hpp", "pairing29.hip.hpp", "pairing29_pair.hip.hpp", "wide29.hip.hpp", "curve29_quad.hip.hpp", "curve29_oct.hip.hpp",
           "wire29.hip.hpp", "h2c29.hip.hpp", "xmd29.hip.hpp", "msm29.hip.hpp", "group29.hip.hpp", "fr29.hip.hpp", "segred29.hip.hpp", "gtmexp29.hip.hpp", "gmsm29.hip.hpp", "subset29.hip.hpp", "transcript29.hip.hpp", "chacha29.hip.hpp", "share29.hip.hpp", "recon29.hip.hpp", "forest29.hip.hpp", "select29.hip.hpp", "formula29.hip.hpp", "fbindex29.hip.hpp", "lsss29.hip.hpp", "mask29.hip.hpp", "frdot29.hip.hpp", "member29.hip.hpp", "gtfixed29.hip.hpp", "openings29.hip.hpp", "bn254_constants.hip.hpp", "bn254_constants29.hip.hpp"]
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC"]
# host-only measurement program over the C ABI (bench.py runs it: calls/s of concurrent one-element calls); built next to the library
CALLS_SRC = os.path.join(HERE, "..", "tools", "concurrent_calls.cpp")
CALLS_EXE = os.path.join(HERE, "gpbc_concurrent_calls")


def _source_hash():
    h = hashlib.sha256(" ".join(FLAGS).encode())
    deps = [os.path.join(CSRC, f) for f in ALL_UNITS + GTFIXED_SOURCES + OPENINGS_SOURCES + HEADERS] + [os.path.join(HERE, "..", "include", name) for name in ("gpbc_bn254.h", "gpbc_bn254_ext.h", "gpbc_bn254_subset.h", "gpbc_bn254_hash.h", "gpbc_bn254_share.h", "gpbc_bn254_indexed.h", "gpbc_bn254_recon.h", "gpbc_bn254_select.h", "gpbc_bn254_formula.h", "gpbc_bn254_random.h", "gpbc_bn254_forest.h", "gpbc_bn254_mask.h", "gpbc_bn254_verify.h", "gpbc_bn254_member.h", "gpbc_bn254_gtfixed.h", "gpbc_bn254_openings.h")] + [CALLS_SRC]
    for d in deps:
        with open(d, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def _stale():
    """Content hash, not mtimes: the GPU box receives a copy of the tree whose timestamps are not the build's."""
    if not os.path.exists(LIB) or not os.path.exists(STAMP) or not os.path.exists(CALLS_EXE):
        return True
    with open(STAMP) as f:
        return f.read().strip() != _source_hash()


def _check_isa(tmp):
    """Refuse device code that contains v_subrev_*_dpp.  The compiler folds `a - swap(b)` (swap = a single-use DPP lane move) into
    v_subrev_u32_dpp assuming src1 - dpp(src0); gfx950 computes dpp(src1) - src0 (tools/subdpp_probe.hip: every lane wrong, for the
    compiler's output and for the hand-written instruction).  csrc/tower29_pair.hip.hpp subtracts on the sending lane instead; this
    check keeps a later edit from re-introducing the pattern silently (the host interval harness has no DPP and cannot see it)."""
    import glob
    import re
    bad = []
    for s in ALL_UNITS + GTFIXED_SOURCES + OPENINGS_SOURCES:
        unit = s.replace(".hip", "")
        files = glob.glob(os.path.join(tmp, unit, "*gfx950*.s"))
        if not files:                                   # a check that scanned nothing has checked nothing
            raise RuntimeError("no gfx950 ISA file (-save-temps) found for %s under %s: the v_subrev_*_dpp fence cannot run" % (s, os.path.join(tmp, unit)))
        for f in files:
            with open(f, errors="replace") as fh:
                n = len(re.findall(r"^\s+v_subb?rev\w*_dpp\b", fh.read(), flags=re.M))
            if n:
                bad.append("%s: %d" % (os.path.basename(f), n))
    if bad:
        raise RuntimeError("device ISA contains v_subrev_*_dpp (wrong on gfx950, see _build._check_isa): " + ", ".join(bad))


def build_library(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 -> gopairingbasedcryptography_amd/libgpbc_bn254.so; returns its path."""
    if not force and not _stale():
        return LIB
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory(prefix="gpbc_build_") as tmp:
        procs = []
        for s in ALL_UNITS + GTFIXED_SOURCES + OPENINGS_SOURCES:
            unit = os.path.join(tmp, s.replace(".hip", ""))
            os.makedirs(unit)
            obj = os.path.join(unit, s.replace(".hip", ".o"))
            cmd = [hipcc] + FLAGS + ["-save-temps", "-c", os.path.join(CSRC, s), "-o", obj]      # temps (the device ISA among them) land in cwd = unit
            if verbose:
                print(" ".join(cmd))
            log = open(os.path.join(unit, "stderr.txt"), "w+")
            procs.append((cmd, obj, subprocess.Popen(cmd, cwd=unit, stderr=None if verbose else log), log))
        objs = []
        for cmd, obj, p, log in procs:
            if p.wait() != 0:
                for _, _, q, _ in procs:
                    if q.poll() is None:
                        q.kill()
                log.seek(0)
                raise RuntimeError("%s failed (exit %d):\n%s" % (" ".join(cmd), p.returncode, log.read()[-8000:]))
            objs.append(obj)
        _check_isa(tmp)
        link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(link))
        subprocess.check_call(link)
    calls = ["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(HERE, "..", "include"), CALLS_SRC, "-L" + HERE, "-lgpbc_bn254",
             "-Wl,-rpath,$ORIGIN", "-o", CALLS_EXE]
    if verbose:
        print(" ".join(calls))
    subprocess.check_call(calls)
    with open(STAMP, "w") as f:
        f.write(_source_hash() + "\n")
    return LIB


if __name__ == "__main__":
    print(build_library(force=True, verbose=True))
