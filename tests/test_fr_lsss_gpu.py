"""The LSSS-weight kernel on the MI355X (run with -m gpu): k_fr_lsss_weights through the host-pointer and the device entry.

  * the case lists of tests/fr_lsss_cases.py (sizes, policies, pivoting, edge values, dense systems, both broadcast forms) against
    the elimination in Python integers, host arrays and CUDA tensors;
  * nested Python integers in; out= / ok_out= into caller buffers with a guard row and a guard byte behind them;
  * once more in a process bound to the device list {0, 0} with enough systems to cross the shard split;
  * chaining: the weights as device scalars into g1_scalar_mul."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import fr_cases as fc
import fr_lsss_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from gopairingbasedcryptography_amd import _build, bn254
    _build.build_library()
    bn254.init(0)
    return bn254


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_cases_host_and_device(eng):
    import torch
    cases = lc.all_cases()
    assert lc.run_cases(lc.engine_call(eng), cases) == []
    assert lc.run_cases(lc.engine_call(eng, put=to_dev, back=lambda t: t.cpu().numpy()), cases) == []
    torch.cuda.synchronize()


def test_python_ints_in(eng):
    c = lc.policy_cases()[0]                                         # "and-or": one nested matrix, four masks
    assert c["label"] == "and-or"
    w, ok = eng.fr_lsss_weights(c["matrices"][0], held=c["held"])
    assert w.shape == (4, 4, 32) and ok.tolist() == [1, 1, 0, 1] and (fc.ints(w), ok.tolist()) == lc.expected(c)
    c = lc.value_cases()[0]                                          # a matrix per mask, rows and cols derived
    w, ok = eng.fr_lsss_weights(c["matrices"], held=c["held"])
    assert (fc.ints(w), ok.tolist()) == lc.expected(c)


def test_out_into_caller_buffers(eng):
    """out= and ok_out= on host arrays and on CUDA tensors: exactly the caller's rows are filled (the guards stay as they were)"""
    import torch
    c = lc.large_k_cases()[3]                                        # 17 x 4, 70 systems
    k, rows, cols = c["k"], c["rows"], c["cols"]
    m, h = lc.flat(c["matrices"]).reshape(-1), lc.mask_bytes(c["held"])
    host, hok = np.full((k * rows + 1) * 32, 0x5A, dtype=np.uint8), np.full(k + 1, 0x5A, dtype=np.uint8)
    w, ok = eng.fr_lsss_weights(m, rows, cols, h, out=host[:k * rows * 32], ok_out=hok[:k])
    assert (fc.ints(w), ok.tolist()) == lc.expected(c) and (host[k * rows * 32:] == 0x5A).all() and hok[k] == 0x5A
    buf, bok = torch.full(((k * rows + 1) * 32,), 0x5A, dtype=torch.uint8, device="cuda"), torch.full((k + 1,), 0x5A, dtype=torch.uint8, device="cuda")
    w, ok = eng.fr_lsss_weights(to_dev(m), rows, cols, to_dev(h), out=buf[:k * rows * 32], ok_out=bok[:k])
    assert (fc.ints(w.cpu().numpy()), ok.cpu().tolist()) == lc.expected(c) and bool((buf[k * rows * 32:] == 0x5A).all()) and int(bok[k]) == 0x5A


def test_host_entry_across_the_shard_split():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fr_lsss_cases.py"), "0", "0"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "devices 2 failures []" in r.stdout


def test_weights_chain_into_g1_scalar_mul(eng, oracle):
    """[w_x] g1 for the masks of the 8-of-16 policy: the device weights as the scalars of g1_scalar_mul equal the oracle's
    multiplication by Python's weights"""
    c = lc.policy_cases()[6]
    assert c["label"] == "shamir-8-of-16"
    want_w, want_ok = lc.expected(c)
    w, ok = eng.fr_lsss_weights(to_dev(lc.flat(c["matrices"]).reshape(-1)), 16, 8, to_dev(lc.mask_bytes(c["held"])))
    assert fc.ints(w.cpu().numpy()) == want_w and ok.cpu().tolist() == want_ok
    g1 = eng.generators()[0]
    got = eng.g1_scalar_mul(to_dev(np.tile(g1, len(want_w))), w.reshape(-1))
    want = np.asarray(oracle.g1_scalar_mul(g1, fc.rows(want_w).reshape(-1), threads=4)).reshape(-1, 64)
    assert (got.cpu().numpy().reshape(-1, 64) == want).all()
