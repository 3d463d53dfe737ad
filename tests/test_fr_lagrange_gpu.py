"""The Lagrange basis kernel on the MI355X (run with -m gpu): k_fr_lagrange_basis through the host-pointer and the device entry.

  * the case lists of tests/fr_lagrange_cases.py (sizes, the shapes at which the launch changes, edge values, every broadcast form)
    and B = m = 1024 against Python's integers, host arrays and CUDA tensors;
  * out= into a caller's buffer with a guard row behind it;
  * once more in a process bound to the device list {0, 0} with enough rows to cross the shard split;
  * chaining: the coefficients as device scalars into g1_scalar_mul."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import fr_cases as fc
import fr_lagrange_cases as lc

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
    cases = lc.all_cases() + [lc.big_case()]
    assert lc.run_cases(lc.engine_call(eng), cases) == []
    assert lc.run_cases(lc.engine_call(eng, put=to_dev, back=lambda t: t.cpu().numpy()), cases) == []
    torch.cuda.synchronize()


def test_python_ints_in(eng):
    c = lc.value_cases()[3]                                          # "equal-mod-r": nested ints, nodes omitted, one x per row
    assert c["label"] == "equal-mod-r"
    got = eng.fr_lagrange_basis(c["set"], x=c["x"])
    assert got.shape == (4, 6, 32) and fc.ints(got) == lc.expected(c)


def test_out_into_caller_buffers(eng):
    """out= on a host array and on a CUDA tensor: exactly the caller's rows are filled (a guard row behind them stays as it was)"""
    import torch
    c = lc.geometry_cases()[1]                                       # B = 17, m = 5, 70 rows
    k, m = c["k"], c["m"]
    s, nd, x = lc.flat(c["set"]).reshape(-1), lc.flat(c["nodes"]).reshape(-1), fc.rows(c["x"]).reshape(-1)
    host = np.full((k * m + 1) * 32, 0x5A, dtype=np.uint8)
    got = eng.fr_lagrange_basis(s, c["B"], nd, m, x, out=host[:k * m * 32])
    assert fc.ints(got) == lc.expected(c) and (host[k * m * 32:] == 0x5A).all()
    buf = torch.full(((k * m + 1) * 32,), 0x5A, dtype=torch.uint8, device="cuda")
    got = eng.fr_lagrange_basis(to_dev(s), c["B"], to_dev(nd), m, to_dev(x), out=buf[:k * m * 32])
    assert fc.ints(got.cpu().numpy()) == lc.expected(c) and bool((buf[k * m * 32:] == 0x5A).all())


def test_host_entry_across_the_shard_split():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fr_lagrange_cases.py"), "0", "0"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "devices 2 failures []" in r.stdout


def test_coefficients_chain_into_g1_scalar_mul(eng, oracle):
    """[Delta_i(0)] g1 for 64 sets of 16: the device coefficients as the scalars of g1_scalar_mul equal the oracle's multiplication by
    Python's coefficients"""
    sets = lc.rand_rows("chain", 64, 16)
    want_k = [lc.basis(S, t, 0) for S in sets for t in S]
    delta = eng.fr_lagrange_basis(to_dev(lc.flat(sets).reshape(-1)), 16)
    assert fc.ints(delta.cpu().numpy()) == want_k
    g1 = eng.generators()[0]
    got = eng.g1_scalar_mul(to_dev(np.tile(g1, len(want_k))), delta.reshape(-1))
    want = np.asarray(oracle.g1_scalar_mul(g1, fc.rows(want_k).reshape(-1), threads=4)).reshape(-1, 64)
    assert (got.cpu().numpy().reshape(-1, 64) == want).all()
