/* Sums in Fr and verdicts in GT for batch verification, entries of libgpbc_bn254.so added after the main header (gpbc_bn254.h) was frozen at
 * gpbc_abi_version() 8, beside the other headers of its kind (gpbc_bn254_ext.h, gpbc_bn254_subset.h, gpbc_bn254_hash.h, ...).  Everything
 * the main header says about status codes, gpbc_last_error(), devices, host-pointer entries (synchronous) and *_dev entries (device
 * pointers and a `stream`, asynchronous) holds here; gpbc_verify_version() counts the revisions of this file.
 *
 * Entry map (what replaces what):
 *   out[s] = sum_i a[i] b[i] mod r over a segment, out[s] = sum_i a[i]                gpbc_fr_dot_segments(_dev)
 *       the scalar sums of a batch verifier.  The reference verifies one signature per call (signature/bls01_signature/bls_signature.go:71-89,
 *       signature/zss04_signature/zss04_signature.go:300-340, signature/bb04_signature/bb04_signature.go:262-295); n of them under one
 *       public key with random weights rho_i need sum rho_i per group beside the weighted point sums.  The same sum is what the
 *       planners' own checks compute: sum_x w_x lambda_x = s after access/tree/access_tree_node.go:96-164 and
 *       access/lsss/lewko_waters_lsss_matrix.go:131-141.
 *   ok[i] = (a[i] == b[i])                                                             gpbc_gt_equal(_dev)
 *       (*GT).Equal — signature/zss04_signature/zss04_signature.go:337, signature/bb04_signature/bb04_signature.go:292,
 *       gka/agka09/asbb.go:140 — for n elements in one launch, the verdicts left in device memory.
 */
#ifndef GPBC_BN254_VERIFY_H
#define GPBC_BN254_VERIFY_H
#include "gpbc_bn254.h"
#ifdef __cplusplus
extern "C" {
#endif

int gpbc_verify_version(void);                                 /* 1 */

/* Reductions in Fr: out[s] = sum over i in [seg_off[s], seg_off[s+1]) of a[i] * b[i] mod r.  The shape and the rules of
 * gpbc_gt_multi_exp, with sums for products and products for powers:
 *   a, b, out: the ABI's scalar format (32 bytes, little-endian).  Inputs may be any value below 2^256 and act as their residue; outputs
 *   are canonical in [0, r).  An empty segment gives 0.
 *   b: nb == n, one per element; or nb == n / n_seg, ONE list for all segments, each of exactly nb elements; or b == NULL with
 *   nb == 0: the plain sum of a.
 * seg_off: n_seg + 1 non-decreasing entries from 0 to n; the host entry validates it (and that a shared list fits every segment), the
 * _dev entry clamps every offset to n and ends a segment after nb elements of a shared list, so a malformed table gives wrong sums but
 * never an out-of-range read — gpbc_check_segments_dev validates a device table.  out (n_seg scalars) must not overlap a or b.  Anything
 * else is GPBC_ERR_INVALID_ARG before any launch, with nothing written.  n_seg == 0 is a no-op.
 * Workspace: gpbc_fr_dot_segments_workspace_bytes(n, n_seg), at most 32 x P bytes of piece values (plus padding to 256) with
 * P = n_seg x J <= 65536 + n_seg pieces and J from n and n_seg alone: bounded whatever the segment lengths are; 0 when no segment is cut.  The workspace
 * must be 16-byte aligned.
 * The _dev entry is stream-ordered and not synchronised; it allocates nothing and reads nothing back.  The host entry stages through
 * the library's device blocks on the calling thread's current device; it is not sharded over devices and not combined across threads. */
int gpbc_fr_dot_segments(const void *a, const void *b, size_t nb, const uint64_t *seg_off, size_t n_seg, void *out);
size_t gpbc_fr_dot_segments_workspace_bytes(size_t n, size_t n_seg);
int gpbc_fr_dot_segments_dev(const void *d_a, const void *d_b, size_t nb, const uint64_t *d_seg_off, size_t n, size_t n_seg,
                             void *d_out, void *d_workspace, size_t workspace_bytes, void *stream);

/* ok_out[i] = 1 iff a[i] == b[j], else 0, with j = i when nb == n and j = 0 when nb == 1: n gnark GT structs (384 bytes each) compared
 * as they are, like (*GT).Equal on canonical elements — no membership test, no reduction.  Rows must be 4-byte aligned (16-byte aligned
 * rows are read 128 bits at a time).  ok_out (n bytes) must not overlap an input.  n == 0 is a no-op; nb other than n or 1, or a null
 * pointer with n > 0, is GPBC_ERR_INVALID_ARG before any launch.  gpbc_gt_equal_dev is ONE launch, ordered on `stream` only, without a
 * workspace; gpbc_gt_equal stages through the library's device blocks and is neither sharded nor combined. */
int gpbc_gt_equal(const void *a, const void *b, size_t nb, size_t n, uint8_t *ok_out);
int gpbc_gt_equal_dev(const void *d_a, const void *d_b, size_t nb, size_t n, uint8_t *d_ok_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
