/* Indexed sums over fixed-base tables and LSSS share generation, entries of libgpbc_bn254.so added after the main header (gpbc_bn254.h) was
 * frozen at gpbc_abi_version() 8, beside gpbc_bn254_ext.h, gpbc_bn254_subset.h, gpbc_bn254_hash.h and gpbc_bn254_share.h.  Everything the
 * main header says about status codes, gpbc_last_error(), devices, host-pointer entries (synchronous) and *_dev entries (device pointers and
 * a `stream`, stream-ordered, not synchronised) holds here; gpbc_indexed_version() counts the revisions of this file.
 *
 * Scalars are the ABI's one scalar format: 32 bytes, little-endian.  Every entry is one kernel launch and needs no workspace.
 *
 * Entry map (what replaces what):
 *   sums of one or two public bases per output  gpbc_fixed_base_indexed(_dev)
 *       C_x = [lambda_x] g1^a + [-r_x] h_rho(x)   cpabe/waters11/waters11_cpabe.go:211-228 (Encrypt)
 *       K_x = [t] h_x                             cpabe/waters11/waters11_cpabe.go:153-156 (KeyGenerate)
 *       c3x = [r_x] g2^y_rho(x) + [omega_x] g2    dabe/lw11_dabe.go:154-157 (Encrypt)
 *       Cy' = [q_y(0)] H1(att(y))                 cpabe/bsw07/bsw07_cpabe.go Encrypt, the loop over the leaves
 *   lambda_x = M_x . v for a batch of vectors   gpbc_fr_lsss_shares(_dev)
 *       LewkoWatersLsssMatrix.ComputeVector       access/lsss/lewko_waters_lsss_matrix.go:131-141
 */
#ifndef GPBC_BN254_INDEXED_H
#define GPBC_BN254_INDEXED_H
#include "gpbc_bn254.h"
#ifdef __cplusplus
extern "C" {
#endif

int gpbc_indexed_version(void);           /* 1 */

/* out[i] = sum_{t < terms} [ scalars[i*terms + t] ] base[ index[(i % n_index_rows)*terms + t] ],  i < n
 *   table:   a gpbc_fixed_base handle (gpbc_g1_/g2_fixed_base_create), G1 or G2; `out` holds n points of its group
 *   index:   n_index_rows x terms uint32; n_index_rows == n gives every output its own row, a smaller value makes the rows periodic
 *            (one policy for a whole batch, the L leaves of a tree).  GPBC_INDEX_NONE means "no term": it is skipped.
 *   scalars: n x terms scalars, any value below 2^256, used as they are through the 32 windows (so [r] B is the point at infinity)
 *   ok_out:  n bytes, or NULL
 * A base that is the point at infinity contributes nothing.  Any other index >= the table's number of bases makes the output row all zero
 * and ok_out[i] = 0 (1 otherwise), the convention of the unmarshal entries and gpbc_fr_poly_quotients; the kernel checks an index before it
 * forms a table address and never reads outside the table.
 * Limits: 1 <= terms <= 16, 1 <= n_index_rows <= n, n * terms < 2^32.  Anything else, a null handle or pointer, a current device other
 * than the table's, or an `out` (or `ok_out`) that overlaps an input is GPBC_ERR_INVALID_ARG before any launch, with nothing written.
 * n == 0 is a no-op.  The host form stages in and out on the table's device; it is neither sharded nor combined across threads. */
#define GPBC_INDEX_NONE 0xffffffffu
int gpbc_fixed_base_indexed(const gpbc_fixed_base *table, const uint32_t *index, size_t n_index_rows, size_t terms,
                            const void *scalars, size_t n, void *out, uint8_t *ok_out);
int gpbc_fixed_base_indexed_dev(const gpbc_fixed_base *table, const uint32_t *d_index, size_t n_index_rows, size_t terms,
                                const void *d_scalars, size_t n, void *d_out, uint8_t *d_ok_out, void *stream);

/* out[j][x] = sum_{c < cols} matrix[j or 0][x][c] * vectors[j][c]  mod r, for k vectors j and the rows x of the matrix
 *   matrix:  n_matrices x rows x cols scalars, row-major (the layout of gpbc_fr_lsss_weights); n_matrices is 1 (one matrix for all) or k
 *   vectors: k x cols scalars;  out: k x rows scalars
 * Entries and vector elements are any value below 2^256 and act as their residue modulo r (-1 arrives as r - 1); outputs are canonical.
 * 1 <= rows, cols <= 64 and k < 2^29; anything else, n_matrices other than 1 or k, a null pointer or an `out` that overlaps an input is
 * GPBC_ERR_INVALID_ARG before any launch, with nothing written.  k == 0 is a no-op.
 * The host form is sharded over the bound devices by vectors; a matrix given once travels whole to every shard. */
int gpbc_fr_lsss_shares(const void *matrix, size_t n_matrices, size_t rows, size_t cols, const void *vectors, size_t k, void *out);
int gpbc_fr_lsss_shares_dev(const void *d_matrix, size_t n_matrices, size_t rows, size_t cols, const void *d_vectors, size_t k,
                            void *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
