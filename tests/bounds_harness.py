"""The one way into tools/libgpbc_bounds.so, the device headers compiled for the host with -DGPBC_BOUNDS (tools/bounds_check.cpp): the
build recipe, the C signature of every hc_* entry, and load(), which builds the library when it is older than its sources and declares
every entry.  Test modules take the `hc` fixture from here (not collected: no test_ prefix)."""
import ctypes
import glob
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join("tools", "bounds_check.cpp")
SO = os.path.join("tools", "libgpbc_bounds.so")
# the compile command up to `-o <output> <source>`
RECIPE = ["g++", "-O2", "-pthread", "-std=c++17", "-DGPBC_BOUNDS", "-shared", "-fPIC"]

# The C signatures of the extern "C" entries of tools/bounds_check.cpp, in its order, in the notation of _lib.SIGNATURES
# (p pointer, z size_t, i int) with  q uint64_t by value,  d double  and  v void (a return only).  load() declares every restype and
# argtypes from this table; tests/test_bounds_harness.py holds it against the definitions in the source and the exports of the library.
HC_SIGNATURES = {
    "hc_subset_sum": "v:ipzppzzp", "hc_subset_shape": "v:zzp", "hc_multi_scalar_mul": "v:ippzpzzp", "hc_gmsm_group": "i:i",
    "hc_pair_wide": "v:ppzpi", "hc_gt_exp_wide": "v:ppzp", "hc_pair": "v:ppzp", "hc_miller": "v:ppzp", "hc_final_exp": "v:pzp",
    "hc_g1_mul": "v:ppzp", "hc_g2_mul": "v:ppzp", "hc_glv_split": "v:pzp", "hc_g2_mul_glv": "v:ppzp", "hc_gls_split": "v:pzp", "hc_fp_mul": "v:ppzp",
    "hc_fp_inv": "v:pzpp", "hc_fp_legendre": "v:pzp", "hc_gt_mul": "v:ppzp", "hc_gt_div": "v:ppzp", "hc_gt_inv": "v:pzp", "hc_gt_sqr": "v:pzpi",
    "hc_pair_lanes": "v:ppzpi", "hc_sparse_products": "v:ppzipp", "hc_pair_lanes_multi": "v:ppzp", "hc_pair_fixed_q": "v:ppzpi",
    "hc_gt_pair_ops": "v:ppzppppp", "hc_gt_exp_pair": "v:ppzp", "hc_final_exp_forms": "v:pzpi", "hc_gt_is_cyclotomic": "v:pzp", "hc_gt_multi_exp_pair": "v:ppzpzzp", "hc_wire_encode": "v:ipzip",
    "hc_wire_decode": "v:ipizpp", "hc_hash_g1_gt_gt_to_fr": "v:pppzp", "hc_sha256": "v:ppzzip", "hc_fe_sqrt": "v:pzpp", "hc_f2_sqrt": "v:pzpp",
    "hc_map_fields": "v:ipzp", "hc_g1_fb_msm": "v:pzpzp", "hc_group_op": "i:iippzzpi", "hc_group_k": "i:i", "hc_msm": "v:ippzip",
    "hc_fr_op": "i:ippzzpi", "hc_fr_inv_k": "i:", "hc_fr_poly_from_roots": "i:pzzp", "hc_fr_poly_quotients": "i:ppzzzpp",
    "hc_fr_lagrange_basis": "i:pzzpzzpzzpi", "hc_fr_lagrange_g": "i:", "hc_fr_lagrange_launch": "i:pzzpzzpzzpp", "hc_fr_lsss_weights": "i:pzzzpzpp",
    "hc_fr_lsss_launch": "i:pzzzpzppp", "hc_fr_poly_eval": "i:pzzpzzzpp", "hc_fr_share_plan": "i:pzpp", "hc_fr_share_tree": "i:pzppzpp",
    "hc_fr_tree_weights": "i:pzpzppp", "hc_fr_lsss_shares": "i:pzzzpzpp", "hc_fr_find_common": "i:pzzpzzzppppp",
    "hc_fr_lsss_from_formula": "i:pzzzzppppip", "hc_formula_select": "i:pzzpzzppp", "hc_chacha_blocks": "i:pqqzpi", "hc_fr_wide_reduce": "i:pzpii",
    "hc_fr_random": "i:pqqzp", "hc_fr_dot_segments": "i:ppzpzzpp", "hc_fr_dot_shape": "v:p", "hc_fb_indexed": "i:ipzpzzpzzppp", "hc_mads_take": "d:",
    "hc_stats": "v:p", "hc_fr_forest_plan": "i:ppzppp", "hc_fr_share_forest": "i:ppzpppzppp", "hc_fr_forest_weights": "i:ppzppzppp",
    "hc_g1_is_on_curve": "v:pzp", "hc_g2_is_in_subgroup": "v:pzpi", "hc_gt_is_in_subgroup": "v:pzpi", "hc_gt_fb_build": "i:pzp",
    "hc_gt_fb_indexed": "i:pzpzzpzpp", "hc_fr_poly_from_roots_segments": "i:ppzzp", "hc_fb_openings": "i:ipzpppzzpp", "hc_opn_shape": "v:zzp",
    "hc_fe_primitive": "i:ippzippp",
}
# every pointer is a c_void_p: it takes ints, None, ctypes arrays and string buffers, byref() and ndarray.ctypes.data_as() alike
CTYPES = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int, "q": ctypes.c_uint64, "d": ctypes.c_double, "v": None}

_lib = None


def build():
    """compile to a name of its own, then move into place: a process that loads the library while another one builds it sees the old
    file or the new one, never half of one"""
    so = os.path.join(ROOT, SO)
    tmp = "%s.%d.tmp" % (so, os.getpid())
    try:
        subprocess.check_call(RECIPE + ["-o", tmp, os.path.join(ROOT, SRC)])
        os.replace(tmp, so)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def load():
    """tools/libgpbc_bounds.so, rebuilt when it is older than bounds_check.cpp or any csrc/*.hpp, loaded once per process, with every
    hc_* entry declared from HC_SIGNATURES"""
    global _lib
    if _lib is None:
        so = os.path.join(ROOT, SO)
        sources = [os.path.join(ROOT, SRC)] + glob.glob(os.path.join(ROOT, "gopairingbasedcryptography_amd", "csrc", "*.hpp"))
        if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in sources):
            build()
        lib = ctypes.CDLL(so)
        for name, sig in HC_SIGNATURES.items():
            ret, params = sig.split(":")
            fn = getattr(lib, name)
            fn.restype = CTYPES[ret]
            fn.argtypes = [CTYPES[k] for k in params]
        _lib = lib
    return _lib


@pytest.fixture(scope="module")
def hc():
    return load()
