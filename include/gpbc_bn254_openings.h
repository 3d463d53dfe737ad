/* Opening proofs over ragged batches, entries of libgpbc_bn254.so added after the main header (gpbc_bn254.h) was frozen at gpbc_abi_version() 8,
 * beside gpbc_bn254_indexed.h and gpbc_bn254_gtfixed.h.  Everything the main header says about status codes, gpbc_last_error(), devices,
 * host-pointer entries (synchronous) and *_dev entries (device pointers and a `stream`, stream-ordered, not synchronised) holds here;
 * gpbc_openings_version() counts the revisions of this file.
 *
 * Scalars are the ABI's one scalar format: 32 bytes, little-endian, any value below 2^256 acting as its residue modulo r.  Points are gnark's
 * in-memory affine structs (G1 64 bytes, G2 128 bytes).
 *
 * Segments are described as gpbc_multi_pair_hostseg_dev describes them: `seg_off` is an array in HOST memory in both forms, k + 1
 * non-decreasing uint64 with seg_off[0] == 0 and seg_off[k] == n, the number of roots / identities.  The library copies what it needs of it
 * before it returns; segment j is the elements [seg_off[j], seg_off[j+1]) and has m_j of them.
 *
 * Entry map (what replaces what): the batch polynomial of 1 <= m <= B identities and the opening proof of every one of them,
 *       Digest, Decrypt (pi = [f(tau) / (tau - id)]_2)        bibe/gwww25_bibe/gwww25_bibe.go:162-176, :211-228
 *       Digest, Decrypt (pi = [f(tau) / (tau - id)]_1)        bibe/afp25_bibe/afp25_bibe.go:293-305, :369-393
 * Before, gpbc_fr_poly_from_roots took one batch size B per call, and the quotient rows of gpbc_fr_poly_quotients (stride scalars per
 * identity) went through device memory into gpbc_fixed_base_msm; here a lane makes the quotient's coefficients as it adds their terms.
 */
#ifndef GPBC_BN254_OPENINGS_H
#define GPBC_BN254_OPENINGS_H
#include "gpbc_bn254.h"
#ifdef __cplusplus
extern "C" {
#endif

int gpbc_openings_version(void);          /* 1 */

/* Row j of coeffs_out (stride scalars) = the m_j + 1 coefficients of prod_{i in segment j} (X - roots[i]), constant term first, canonical,
 * then stride - m_j - 1 zeros; an empty segment gives the polynomial 1.  On segments that all hold B roots and stride = B + 1 the output
 * is byte for byte that of gpbc_fr_poly_from_roots.
 * Limits: m_j <= 1024, m_j + 1 <= stride <= 2^24, k < 2^31.  Anything else, a table that does not start at 0 or decreases, or a null
 * pointer (roots may be null when n == 0) is GPBC_ERR_INVALID_ARG before any launch, with nothing written.  k == 0 is a no-op. */
int gpbc_fr_poly_from_roots_segments(const void *roots, const uint64_t *seg_off, size_t k, size_t stride, void *coeffs_out);
int gpbc_fr_poly_from_roots_segments_dev(const void *d_roots, const uint64_t *seg_off, size_t k, size_t stride, void *d_coeffs_out, void *stream);

/* Opening proofs against a fixed-base table (gpbc_g1/g2_fixed_base_create) of nbase bases in which base c stands for [tau^c]:
 *   coeffs:  k rows of nbase scalars, row j = f_j as the entry above writes it with stride = nbase
 *   ids:     n scalars; identity i of segment j has q_i(X) = f_j(X) / (X - ids[i]), of degree m_j - 1
 *   out:     n affine points of the table's group, out[i] = sum_{c < m_j} q_(i,c) base[c]
 *   ok_out:  n bytes or NULL; ok_out[i] = 1 iff f_j(ids[i]) == 0 AND q_i(ids[i]) != 0, that is, the identity is a root of its batch's
 *            polynomial exactly once (the reference removes every identity equal to id and fails unless exactly one was removed; a repeated
 *            identity is a double root).  Otherwise out[i] is all zero and ok_out[i] = 0.
 * No quotient row is written to memory.  The device form needs gpbc_fixed_base_openings_workspace_bytes(table, n) bytes of workspace (0:
 * none, and d_workspace may be null); the host form stages in and out on the table's device and is neither sharded nor combined.
 * Limits: m_j + 1 <= nbase, n < 2^31.  Anything else, a malformed table, a null handle or pointer (other than ok_out), a current device
 * other than the table's, or an `out` / `ok_out` that overlaps an input or the other output is GPBC_ERR_INVALID_ARG before any launch, with
 * nothing written; a workspace that is too small is GPBC_ERR_WORKSPACE.  k == 0 or n == 0 is a no-op. */
size_t gpbc_fixed_base_openings_workspace_bytes(const gpbc_fixed_base *table, size_t n);
int gpbc_fixed_base_openings(const gpbc_fixed_base *table, const void *coeffs, const void *ids, const uint64_t *seg_off, size_t k, void *out, uint8_t *ok_out);
int gpbc_fixed_base_openings_dev(const gpbc_fixed_base *table, const void *d_coeffs, const void *d_ids, const uint64_t *seg_off, size_t k, void *d_out, uint8_t *d_ok_out,
                                 void *d_workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
