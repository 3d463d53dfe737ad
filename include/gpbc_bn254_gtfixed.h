/* Fixed-base exponentiation in GT, entries of libgpbc_bn254.so added after the main header (gpbc_bn254.h) was frozen at gpbc_abi_version() 8,
 * beside gpbc_bn254_indexed.h and gpbc_bn254_member.h.  Everything the main header says about status codes, gpbc_last_error(), devices,
 * host-pointer entries (synchronous) and *_dev entries (device pointers and a `stream`, stream-ordered, not synchronised) holds here;
 * gpbc_gtfixed_version() counts the revisions of this file.
 *
 * GT elements are gnark's in-memory structs (384 bytes, GPBC_GT_BYTES); scalars are the ABI's one scalar format: 32 bytes, little-endian.
 * An indexed product is one kernel launch and needs no workspace.
 *
 * Entry map (what replaces what): a public GT element raised to a fresh scalar per item, gpbc_gt_fixed_base_indexed(_dev) with terms = 1
 *       e(g1, g2)^s                               ibe/bb04_sibe/bb04_sibe.go:195-200 (Encrypt)
 *       e(g1^alpha, g2)^t                         ibe/bb04_ibe/bb04_ibe.go:181-189, ibe/waters05_ibe/waters05_ibe.go:214 (Encrypt)
 *       e(g, g)^s,  e(g, h1)^-s                   ibe/gentry06_ibe/gentry06_ibe.go:192-245 (Encrypt: v and w)
 *   and a product of two such powers, terms = 2
 *       e(g, h2)^s e(g, h3)^(s beta)              ibe/gentry06_ibe/gentry06_ibe.go:192-245 (Encrypt: y)
 * Before, the base was replicated n times and went through gpbc_gt_exp_batch: 252 squarings and 77 products per item; a term here is 32
 * products against a table in device memory and no squarings.
 */
#ifndef GPBC_BN254_GTFIXED_H
#define GPBC_BN254_GTFIXED_H
#include "gpbc_bn254.h"
#include "gpbc_bn254_indexed.h"
#ifdef __cplusplus
extern "C" {
#endif

int gpbc_gtfixed_version(void);           /* 1 */

/* Window tables of nbase public GT elements in device memory: base_j ^ (d 2^(8w)) for d = 0 .. 255 and w = 0 .. 31, 4 MiB per base
 * (gpbc_gt_fixed_base_table_bytes; 0 when the size does not fit a size_t).  A base is ANY Fp12 element, as for gnark's GT.Exp — one, a
 * pairing value, a Miller-loop value, zero; nothing is assumed about its order.
 *   create:      `bases` on the host, nbase x 384 bytes; the table is complete on return
 *   create_dev:  `d_bases` in device memory; the build is enqueued on `stream` and NOT synchronised — d_bases must stay as it is until the
 *                build has run, and work that uses the table is ordered behind it on `stream` (or after a synchronisation)
 *   destroy:     synchronises the table's device, then frees; a null handle is a no-op
 * The handle belongs to the device that was current when it was made.  nbase == 0, a null pointer or a table too large to address is
 * GPBC_ERR_INVALID_ARG with *out = NULL. */
typedef struct gpbc_gt_fixed_base gpbc_gt_fixed_base;
size_t gpbc_gt_fixed_base_table_bytes(size_t nbase);
int gpbc_gt_fixed_base_create(const void *bases, size_t nbase, gpbc_gt_fixed_base **out);
int gpbc_gt_fixed_base_create_dev(const void *d_bases, size_t nbase, void *stream, gpbc_gt_fixed_base **out);
int gpbc_gt_fixed_base_destroy(gpbc_gt_fixed_base *table);

/* out[i] = prod_{t < terms} base[ index[(i % n_index_rows)*terms + t] ] ^ scalars[i*terms + t],  i < n      (the contract of
 * gpbc_fixed_base_indexed, in GT)
 *   index:   n_index_rows x terms uint32; n_index_rows == n gives every output its own row, a smaller value makes the rows periodic.
 *            GPBC_INDEX_NONE means "no term": it is skipped, and a row of nothing else gives one.
 *   scalars: n x terms scalars, any value below 2^256, used as the integers they are: the result is gnark's GT.Exp(base, k) for every
 *            non-zero base, whatever its order.  A zero base gives zero for k > 0 and one for k = 0.
 *   out:     n x 384 bytes;  ok_out: n bytes, or NULL
 * Any other index >= the table's number of bases makes the output row all zero and ok_out[i] = 0 (1 otherwise); the kernel checks an index
 * before it forms a table address and never reads outside the table.
 * Limits: 1 <= terms <= 16, 1 <= n_index_rows <= n, n * terms < 2^32.  Anything else, a null handle or pointer, a current device other
 * than the table's, or an `out` (or `ok_out`) that overlaps an input is GPBC_ERR_INVALID_ARG before any launch, with nothing written.
 * n == 0 is a no-op.  The host form stages in and out on the table's device; it is neither sharded nor combined across threads. */
int gpbc_gt_fixed_base_indexed(const gpbc_gt_fixed_base *table, const uint32_t *index, size_t n_index_rows, size_t terms,
                               const void *scalars, size_t n, void *out, uint8_t *ok_out);
int gpbc_gt_fixed_base_indexed_dev(const gpbc_gt_fixed_base *table, const uint32_t *d_index, size_t n_index_rows, size_t terms,
                                   const void *d_scalars, size_t n, void *d_out, uint8_t *d_ok_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
