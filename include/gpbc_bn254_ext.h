/* Extension entries of libgpbc_bn254.so: calls added after the main header (gpbc_bn254.h) was frozen at gpbc_abi_version() 8.
 * Everything the main header says about status codes, gpbc_last_error(), devices, host-pointer entries (synchronous) and *_dev
 * entries (device pointers and a `stream`, asynchronous) holds here; gpbc_ext_version() counts the revisions of this file.
 *
 * Entry map (what replaces what):
 *   sum_x [k_x] P_x per item, P_x ciphertext points in G1    gpbc_g1_multi_scalar_mul(_dev)
 *       S = sum_x [-w_x] C_x of Waters11 Decrypt (cpabe/waters11/waters11_cpabe.go:248-290)
 *   sum_x [k_x] Q_x per item, Q_x ciphertext points in G2    gpbc_g2_multi_scalar_mul(_dev)
 *       sum_x w_x c3x of LW11 Decrypt (dabe/lw11_dabe.go:176-203): prod_x e([w_x]H, c3x) = e(H, sum_x w_x c3x)
 *   sum of the points of every segment, no scalars           the same entries with scalars == NULL, nk == 0
 *   bytes of device memory the _dev entries need             gpbc_multi_scalar_mul_workspace_bytes
 *   what the small-call combiner did since load              gpbc_small_call_stats (revision 2)
 */
#ifndef GPBC_BN254_EXT_H
#define GPBC_BN254_EXT_H
#include "gpbc_bn254.h"
#ifdef __cplusplus
extern "C" {
#endif

int gpbc_ext_version(void);                /* 2 */

/* Reductions in G1 / G2: out[s] = sum over i in [seg_off[s], seg_off[s+1]) of [k_i] P_i, each term with the semantics of
 * gpbc_g1/g2_scalar_mul_batch (scalars are the ABI's one 32-byte little-endian format: any value < 2^256, acting as its residue mod r;
 * points are taken to be on the curve and in the order-r group; the all-zero point is infinity), one chain of doublings shared by four
 * terms.  Outputs are canonical gnark G1Affine / G2Affine: a group element has one such encoding, so the bytes are those of
 * gpbc_g*_scalar_mul_batch folded with gpbc_g*_add_batch.  An empty segment gives infinity (all zero).
 *   scalars: nk == n, one per term; or nk == n / n_seg, ONE list for all segments, each of exactly nk terms (the weights of one policy
 *   against many ciphertexts); or scalars == NULL with nk == 0: the plain segmented sum — no tables, no doublings.
 * seg_off as for gpbc_gt_multi_exp: n_seg + 1 non-decreasing entries from 0 to n; the host entry validates it (and that a shared list
 * fits every segment), the _dev entry clamps every offset to n and ends a segment after nk terms of a shared list, so a malformed
 * table gives wrong sums but never an out-of-bounds access — gpbc_check_segments_dev validates a device table, and that every
 * segment has nk terms is the caller's promise there.  out (n_seg points) must not overlap the inputs.  n_seg == 0, a null table, a
 * bad nk, an overlap, or a short or missing workspace is GPBC_ERR_INVALID_ARG before any launch, with nothing written.
 * Workspace: gpbc_multi_scalar_mul_workspace_bytes(n, n_seg, is_g2) <= min(P, 131072) x B + W x (P + P / 8) + 768 bytes, with B = 8 832
 * (G1) or 17 152 (G2) bytes per lane block (four tables, the window words of one group, the piece's accumulator), W = 64 or 128 bytes per
 * piece value (P of the first level, at most P / 8 of the next; later levels reuse the two blocks), 768 bytes of padding, and
 * P = n_seg x J <= 131072 + n_seg pieces with J from n and n_seg alone: bounded whatever the segment lengths are.  The workspace must be
 * 16-byte aligned (its rows are read and written 128 bits at a time); one that is not is GPBC_ERR_INVALID_ARG like a short one.
 * The _dev form is stream-ordered on `stream` only and is not synchronised; it reads nothing back and allocates nothing, the
 * workspace is the caller's.  The host form shards by whole segments over the bound devices; it is not combined across calling
 * threads. */
int gpbc_g1_multi_scalar_mul(const void *bases, const void *scalars, size_t nk, const uint64_t *seg_off, size_t n_seg, void *out);
int gpbc_g2_multi_scalar_mul(const void *bases, const void *scalars, size_t nk, const uint64_t *seg_off, size_t n_seg, void *out);
size_t gpbc_multi_scalar_mul_workspace_bytes(size_t n, size_t n_seg, int is_g2);
int gpbc_g1_multi_scalar_mul_dev(const void *d_bases, const void *d_scalars, size_t nk, const uint64_t *d_seg_off, size_t n, size_t n_seg, void *d_out,
                                 void *d_workspace, size_t workspace_bytes, void *stream);
int gpbc_g2_multi_scalar_mul_dev(const void *d_bases, const void *d_scalars, size_t nk, const uint64_t *d_seg_off, size_t n, size_t n_seg, void *d_out,
                                 void *d_workspace, size_t workspace_bytes, void *stream);

/* Host-pointer calls of up to 2 048 units that arrive from several threads while the device is busy share launches (the main header's
 * threading notes; gpbc_msm_stats is the same kind of entry: tests assert which path a workload took).  Process-wide counts since the
 * library was loaded, over all device slots:
 *   batches                   launches of the combiner, counted when a leader has taken its batch and before it launches
 *   calls                     requests served by those batches (calls - batches = requests that rode in another caller's launch)
 *   largest_batch             the most requests in one batch
 *   failed_in_shared_batches  requests that ended with a status other than GPBC_OK in a batch of two or more
 * Needs no device (all zero before any call).  A null pointer is GPBC_ERR_INVALID_ARG with nothing written. */
int gpbc_small_call_stats(uint64_t *batches_out, uint64_t *calls_out, uint64_t *largest_batch_out, uint64_t *failed_in_shared_batches_out);

#ifdef __cplusplus
}
#endif
#endif
