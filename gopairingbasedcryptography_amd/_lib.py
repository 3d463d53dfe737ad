"""ctypes loader for the C-ABI library (include/gpbc_bn254.h).  No fallback: if the HIP library is
missing or no gfx950 device can be bound, every compute call raises."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# GPBC_LIB_PATH: load another build of the same C ABI (kernel-tuning experiments); default is the in-tree library
LIB_PATH = os.environ.get("GPBC_LIB_PATH") or os.path.join(HERE, "libgpbc_bn254.so")

# The C signatures of include/gpbc_bn254.h, in its order: symbol -> "return kind : one kind per parameter".
#   p  pointer (any C type with a `*`)    z  size_t    i  int    l  long    s  const char * (a return only)
# load() declares every restype and argtypes from this table, so a Python int reaches a size_t or pointer parameter at its full
# width and a value of the wrong kind is an ArgumentError at the call, not a truncated argument.
SIGNATURES = {
    "gpbc_init": "i:i", "gpbc_init_devices": "i:pi", "gpbc_num_devices": "i:", "gpbc_device_at": "i:i", "gpbc_set_device": "i:i",
    "gpbc_get_device": "i:", "gpbc_set_host_sharding": "i:i", "gpbc_shutdown": "i:", "gpbc_release_workspaces": "i:",
    "gpbc_last_error": "s:", "gpbc_device_count": "i:", "gpbc_abi_version": "i:", "gpbc_comm_init_all": "i:",
    "gpbc_comm_get_unique_id": "i:p", "gpbc_comm_init_rank": "i:pii", "gpbc_comm_ranks": "i:", "gpbc_comm_rank": "i:",
    "gpbc_comm_destroy": "i:", "gpbc_allgather_dev": "i:pzpp", "gpbc_allgather_all_dev": "i:pzpp", "gpbc_pair_batch": "i:ppzp",
    "gpbc_pair_batch_dev": "i:ppzpp", "gpbc_multi_pair": "i:pppzp", "gpbc_multi_pair_workspace_bytes": "z:zz",
    "gpbc_multi_pair_dev": "i:pppzzppzp", "gpbc_check_segments_dev": "i:pzzp", "gpbc_multi_pair_hostseg_dev": "i:pppzpp",
    "gpbc_multi_pair_fixed_q": "i:ppzzp", "gpbc_multi_pair_fixed_q_dev": "i:ppzzpp", "gpbc_set_multi_pair_chunk": "i:i",
    "gpbc_set_pipelined_miller": "i:i", "gpbc_set_latency_path": "i:l", "gpbc_debug_stale_table_once": "i:",
    "gpbc_pairing_check": "i:pppzp", "gpbc_miller_loop_dev": "i:ppzpp", "gpbc_final_exp_dev": "i:pzpp",
    "gpbc_miller_loop": "i:ppzp", "gpbc_final_exp": "i:pzp", "gpbc_g1_scalar_mul_batch": "i:pzpzp",
    "gpbc_g1_scalar_mul_batch_dev": "i:pzpzpp", "gpbc_g2_scalar_mul_batch": "i:pzpzp", "gpbc_g2_scalar_mul_batch_dev": "i:pzpzpp",
    "gpbc_g1_sum": "i:pzp", "gpbc_g2_sum": "i:pzp", "gpbc_sum_workspace_bytes": "z:zi", "gpbc_g1_sum_dev": "i:pzppzp",
    "gpbc_g2_sum_dev": "i:pzppzp", "gpbc_g1_add_batch": "i:ppzzp", "gpbc_g1_sub_batch": "i:ppzzp", "gpbc_g1_double_batch": "i:pzp",
    "gpbc_g2_add_batch": "i:ppzzp", "gpbc_g2_sub_batch": "i:ppzzp", "gpbc_g2_double_batch": "i:pzp",
    "gpbc_g1_add_batch_dev": "i:ppzzpp", "gpbc_g1_sub_batch_dev": "i:ppzzpp", "gpbc_g1_double_batch_dev": "i:pzpp",
    "gpbc_g2_add_batch_dev": "i:ppzzpp", "gpbc_g2_sub_batch_dev": "i:ppzzpp", "gpbc_g2_double_batch_dev": "i:pzpp",
    "gpbc_g1_scalar_mul_sum": "i:ppzp", "gpbc_g2_scalar_mul_sum": "i:ppzp", "gpbc_g1_scalar_mul_sum_dev": "i:ppzpp",
    "gpbc_g2_scalar_mul_sum_dev": "i:ppzpp", "gpbc_msm_stats": "i:pp", "gpbc_gt_exp_batch": "i:ppzp",
    "gpbc_gt_exp_batch_dev": "i:ppzpp", "gpbc_gt_mul_batch": "i:ppzp", "gpbc_gt_div_batch": "i:ppzp",
    "gpbc_gt_inverse_batch": "i:pzp", "gpbc_gt_mul_batch_dev": "i:ppzpp", "gpbc_gt_div_batch_dev": "i:ppzpp",
    "gpbc_gt_inverse_batch_dev": "i:pzpp", "gpbc_gt_multi_exp": "i:ppzpzp", "gpbc_gt_multi_exp_workspace_bytes": "z:zz",
    "gpbc_gt_multi_exp_dev": "i:ppzpzzppzp", "gpbc_fixed_base_table_bytes": "z:zi", "gpbc_g1_fixed_base_create": "i:pzp",
    "gpbc_g2_fixed_base_create": "i:pzp", "gpbc_fixed_base_create_dev": "i:ipzpp", "gpbc_fixed_base_msm": "i:ppzp",
    "gpbc_fixed_base_msm_workspace_bytes": "z:pz", "gpbc_fixed_base_msm_dev": "i:ppzppzp", "gpbc_fixed_base_destroy": "i:p",
    "gpbc_g1_marshal_batch": "i:pzip", "gpbc_g2_marshal_batch": "i:pzip", "gpbc_gt_marshal_batch": "i:pzp",
    "gpbc_g1_marshal_batch_dev": "i:pzipp", "gpbc_g2_marshal_batch_dev": "i:pzipp", "gpbc_gt_marshal_batch_dev": "i:pzpp",
    "gpbc_g1_unmarshal_batch": "i:pzzpp", "gpbc_g2_unmarshal_batch": "i:pzzpp", "gpbc_gt_unmarshal_batch": "i:pzpp",
    "gpbc_g1_unmarshal_batch_dev": "i:pzzppp", "gpbc_g2_unmarshal_batch_dev": "i:pzzppp", "gpbc_gt_unmarshal_batch_dev": "i:pzppp",
    "gpbc_g1_map_to_curve_batch": "i:pzp", "gpbc_g2_map_to_curve_batch": "i:pzp", "gpbc_g1_map_to_curve_batch_dev": "i:pzpp",
    "gpbc_g2_map_to_curve_batch_dev": "i:pzpp", "gpbc_hash_to_g1": "i:ppzpzp", "gpbc_hash_to_g2": "i:ppzpzp",
    "gpbc_hash_to_field": "i:ppzpzip", "gpbc_hash_to_g1_dev": "i:ppzzpzpp", "gpbc_hash_to_g2_dev": "i:ppzzpzpp",
    "gpbc_hash_to_field_dev": "i:ppzzpzipp", "gpbc_fr_add_batch": "i:ppzzp", "gpbc_fr_sub_batch": "i:ppzzp",
    "gpbc_fr_mul_batch": "i:ppzzp", "gpbc_fr_neg_batch": "i:pzp", "gpbc_fr_inverse_batch": "i:pzp",
    "gpbc_fr_from_mont_batch": "i:pzp", "gpbc_fr_to_mont_batch": "i:pzp", "gpbc_fr_add_batch_dev": "i:ppzzpp",
    "gpbc_fr_sub_batch_dev": "i:ppzzpp", "gpbc_fr_mul_batch_dev": "i:ppzzpp", "gpbc_fr_neg_batch_dev": "i:pzpp",
    "gpbc_fr_inverse_batch_dev": "i:pzpp", "gpbc_fr_from_mont_batch_dev": "i:pzpp", "gpbc_fr_to_mont_batch_dev": "i:pzpp",
    "gpbc_fr_poly_from_roots": "i:pzzp", "gpbc_fr_poly_quotients": "i:ppzzzpp", "gpbc_fr_poly_from_roots_dev": "i:pzzpp",
    "gpbc_fr_poly_quotients_dev": "i:ppzzzppp", "gpbc_fr_lagrange_basis": "i:pzzpzzpzzp",
    "gpbc_fr_lagrange_basis_dev": "i:pzzpzzpzzpp", "gpbc_fr_lsss_weights": "i:pzzzpzpp", "gpbc_fr_lsss_weights_dev": "i:pzzzpzppp",
    "gpbc_profile_begin": "i:p", "gpbc_profile_end": "i:pppip", "gpbc_valu_probe": "i:p", "gpbc_fp_mul_batch": "i:ppzp",
}
EXPORTS = list(SIGNATURES)
# include/gpbc_bn254_ext.h — the entries added since the main header was frozen
EXT_SIGNATURES = {
    "gpbc_ext_version": "i:", "gpbc_g1_multi_scalar_mul": "i:ppzpzp", "gpbc_g2_multi_scalar_mul": "i:ppzpzp",
    "gpbc_multi_scalar_mul_workspace_bytes": "z:zzi", "gpbc_g1_multi_scalar_mul_dev": "i:ppzpzzppzp",
    "gpbc_g2_multi_scalar_mul_dev": "i:ppzpzzppzp", "gpbc_small_call_stats": "i:pppp",
}
# include/gpbc_bn254_subset.h — the bit-selected sums over a fixed set
SUBSET_SIGNATURES = {
    "gpbc_subset_version": "i:", "gpbc_subset_table_bytes": "z:zi", "gpbc_g1_subset_table_create": "i:pzpp",
    "gpbc_g2_subset_table_create": "i:pzpp", "gpbc_subset_table_create_dev": "i:ipzppp", "gpbc_subset_sum": "i:ppzp",
    "gpbc_subset_sum_workspace_bytes": "z:pz", "gpbc_subset_sum_dev": "i:ppzppzp", "gpbc_subset_table_destroy": "i:p",
}
# include/gpbc_bn254_hash.h — SHA-256 on the device with the digest as bytes or as a scalar
HASH_SIGNATURES = {
    "gpbc_hash_version": "i:", "gpbc_sha256_batch": "i:ppzip", "gpbc_sha256_batch_dev": "i:ppzzipp",
    "gpbc_hash_g1_gt_gt_to_fr": "i:pppzp", "gpbc_hash_g1_gt_gt_to_fr_dev": "i:pppzpp",
}
# include/gpbc_bn254_share.h — polynomial evaluation and the shares of a threshold tree in Fr
SHARE_SIGNATURES = {
    "gpbc_share_version": "i:", "gpbc_fr_poly_eval": "i:pzzpzzzp", "gpbc_fr_poly_eval_dev": "i:pzzpzzzpp",
    "gpbc_share_tree_create": "i:pzp", "gpbc_share_tree_destroy": "i:p", "gpbc_share_tree_leaves": "z:p",
    "gpbc_share_tree_coeffs": "z:p", "gpbc_fr_share_tree": "i:pppzp", "gpbc_fr_share_tree_dev": "i:pppzpp",
}
# include/gpbc_bn254_indexed.h — the indexed sums over fixed-base tables and LSSS share generation
INDEXED_SIGNATURES = {
    "gpbc_indexed_version": "i:", "gpbc_fixed_base_indexed": "i:ppzzpzpp", "gpbc_fixed_base_indexed_dev": "i:ppzzpzppp",
    "gpbc_fr_lsss_shares": "i:pzzzpzp", "gpbc_fr_lsss_shares_dev": "i:pzzzpzpp",
}
# include/gpbc_bn254_recon.h — the reconstruction weights of a threshold tree
RECON_SIGNATURES = {
    "gpbc_recon_version": "i:", "gpbc_fr_tree_weights": "i:ppzpp", "gpbc_fr_tree_weights_dev": "i:ppzppp",
}
# include/gpbc_bn254_select.h — the common attributes of a list and a set
SELECT_SIGNATURES = {
    "gpbc_select_version": "i:", "gpbc_fr_find_common": "i:pzzpzzzpppp", "gpbc_fr_find_common_dev": "i:pzzpzzzppppp",
}
# include/gpbc_bn254_formula.h — LSSS matrices and 0 / 1 weights from boolean formulas
FORMULA_SIGNATURES = {
    "gpbc_formula_version": "i:", "gpbc_fr_lsss_from_formula": "i:pzzzzpppp", "gpbc_fr_lsss_from_formula_dev": "i:pzzzzppppp",
    "gpbc_formula_select": "i:pzzpzzpp", "gpbc_formula_select_dev": "i:pzzpzzppp",
}
# include/gpbc_bn254_random.h — ChaCha20 blocks and scalars addressed by (seed, stream, index) and the 64-byte reduction into Fr
RANDOM_SIGNATURES = {
    "gpbc_random_version": "i:", "gpbc_random_bytes": "i:pzzzp", "gpbc_random_bytes_dev": "i:pzzzpp", "gpbc_fr_random": "i:pzzzp",
    "gpbc_fr_random_dev": "i:pzzzpp", "gpbc_fr_set_bytes64": "i:pzp", "gpbc_fr_set_bytes64_dev": "i:pzpp",
}
# include/gpbc_bn254_forest.h — sharing and weights over a forest of threshold trees, a tree per item
FOREST_SIGNATURES = {
    "gpbc_forest_version": "i:", "gpbc_share_forest_create": "i:ppzp", "gpbc_share_forest_destroy": "i:p", "gpbc_share_forest_trees": "z:p",
    "gpbc_share_forest_leaves": "z:p", "gpbc_share_forest_coeffs": "z:p", "gpbc_share_forest_tree_leaves": "z:pz", "gpbc_share_forest_tree_coeffs": "z:pz",
    "gpbc_fr_share_forest": "i:ppppzpp", "gpbc_fr_share_forest_dev": "i:ppppzppp", "gpbc_fr_forest_weights": "i:pppzpp", "gpbc_fr_forest_weights_dev": "i:pppzppp",
}
# include/gpbc_bn254_mask.h — the XOR mask from GT bytes
MASK_SIGNATURES = {
    "gpbc_mask_version": "i:", "gpbc_gt_xor_mask": "i:pppzzpp", "gpbc_gt_xor_mask_dev": "i:pppzzzppp",
}
# include/gpbc_bn254_verify.h — the sums in Fr and the verdicts in GT of batch verification
VERIFY_SIGNATURES = {
    "gpbc_verify_version": "i:", "gpbc_fr_dot_segments": "i:ppzpzp", "gpbc_fr_dot_segments_workspace_bytes": "z:zz", "gpbc_fr_dot_segments_dev": "i:ppzpzzppzp",
    "gpbc_gt_equal": "i:ppzzp", "gpbc_gt_equal_dev": "i:ppzzpp",
}
# include/gpbc_bn254_member.h — IsOnCurve / IsInSubGroup on in-memory G1, G2 and GT elements
MEMBER_SIGNATURES = {
    "gpbc_member_version": "i:", "gpbc_g1_is_on_curve": "i:pzp", "gpbc_g1_is_on_curve_dev": "i:pzpp", "gpbc_g2_is_on_curve": "i:pzp",
    "gpbc_g2_is_on_curve_dev": "i:pzpp", "gpbc_g2_is_in_subgroup": "i:pzp", "gpbc_g2_is_in_subgroup_dev": "i:pzpp",
    "gpbc_gt_is_in_subgroup": "i:pzp", "gpbc_gt_is_in_subgroup_dev": "i:pzpp",
}
# include/gpbc_bn254_gtfixed.h — window tables of public GT elements and indexed products of their powers
GTFIXED_SIGNATURES = {
    "gpbc_gtfixed_version": "i:", "gpbc_gt_fixed_base_table_bytes": "z:z", "gpbc_gt_fixed_base_create": "i:pzp",
    "gpbc_gt_fixed_base_create_dev": "i:pzpp", "gpbc_gt_fixed_base_destroy": "i:p", "gpbc_gt_fixed_base_indexed": "i:ppzzpzpp",
    "gpbc_gt_fixed_base_indexed_dev": "i:ppzzpzppp",
}
# include/gpbc_bn254_openings.h — batch polynomials over segments and opening proofs over fixed-base tables
OPENINGS_SIGNATURES = {
    "gpbc_openings_version": "i:", "gpbc_fr_poly_from_roots_segments": "i:ppzzp", "gpbc_fr_poly_from_roots_segments_dev": "i:ppzzpp",
    "gpbc_fixed_base_openings_workspace_bytes": "z:pz", "gpbc_fixed_base_openings": "i:ppppzpp", "gpbc_fixed_base_openings_dev": "i:ppppzpppzp",
}
# Public header -> its table, in the order the headers were added.  load() declares every table here; a new header is one table above
# and one line here.  tests/test_abi_tables.py holds each table against its header and their union against the library's exports.
HEADERS = {
    "gpbc_bn254.h": SIGNATURES, "gpbc_bn254_ext.h": EXT_SIGNATURES, "gpbc_bn254_subset.h": SUBSET_SIGNATURES,
    "gpbc_bn254_hash.h": HASH_SIGNATURES, "gpbc_bn254_share.h": SHARE_SIGNATURES, "gpbc_bn254_indexed.h": INDEXED_SIGNATURES,
    "gpbc_bn254_recon.h": RECON_SIGNATURES, "gpbc_bn254_select.h": SELECT_SIGNATURES, "gpbc_bn254_formula.h": FORMULA_SIGNATURES,
    "gpbc_bn254_random.h": RANDOM_SIGNATURES, "gpbc_bn254_forest.h": FOREST_SIGNATURES, "gpbc_bn254_mask.h": MASK_SIGNATURES,
    "gpbc_bn254_verify.h": VERIFY_SIGNATURES, "gpbc_bn254_member.h": MEMBER_SIGNATURES, "gpbc_bn254_gtfixed.h": GTFIXED_SIGNATURES,
    "gpbc_bn254_openings.h": OPENINGS_SIGNATURES,
}

# every pointer is a c_void_p: it takes ints, None, c_void_p, ctypes arrays, byref() and ndarray.ctypes.data_as() alike
_CTYPES = {"p": ctypes.c_void_p, "z": ctypes.c_size_t, "i": ctypes.c_int, "l": ctypes.c_long, "s": ctypes.c_char_p}

_lib = None


class EngineError(RuntimeError):
    """Raised when the C ABI returns a negative gpbc_status."""


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EngineError(
                "HIP extension %s is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 and device tensors /
        # streams come from it, so load torch first and let the dynamic loader resolve this library's
        # libamdhip64.so.7 dependency to that already-loaded copy (two runtimes cannot share the GPU).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(LIB_PATH)
        for name, sig in [item for table in HEADERS.values() for item in table.items()]:
            ret, params = sig.split(":")
            fn = getattr(lib, name)
            fn.restype = _CTYPES[ret]
            fn.argtypes = [_CTYPES[k] for k in params]
        _lib = lib
    return _lib


def check(rc):
    if rc < 0:
        raise EngineError("gpbc error %d: %s" % (rc, load().gpbc_last_error().decode()))
    return rc
