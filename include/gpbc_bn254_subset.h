/* Bit-selected sums over a fixed set of points, entries of libgpbc_bn254.so added after the main header (gpbc_bn254.h) was frozen at
 * gpbc_abi_version() 8 and beside the extension header (gpbc_bn254_ext.h, gpbc_ext_version() 2).  Everything the main header says
 * about status codes, gpbc_last_error(), devices, host-pointer entries (synchronous) and *_dev entries (device pointers and a
 * `stream`, asynchronous) holds here; gpbc_subset_version() counts the revisions of this file.
 *
 * Entry map (what replaces what):
 *   U' + sum_{Id[i] = 1} U_i per identity, U_i public G2 points     gpbc_g2_subset_table_create + gpbc_subset_sum(_dev)
 *       the Waters hash of KeyGenerate and Encrypt (ibe/waters05_ibe/waters05_ibe.go:172-179, 226-233), Id[] the 256 bits of
 *       SHA-256(identity), most significant bit of every byte first (NewWaters05IBEIdentity, :290-315): up to 256 G2Affine.Add per call
 *   sum of the keys of the members a bitmap names                   gpbc_g1/g2_subset_table_create + gpbc_subset_sum(_dev)
 *       the aggregation loops of gka/agka09/asbb.go:193-220
 *   bytes of HBM a table takes                                      gpbc_subset_table_bytes
 *   bytes of device memory gpbc_subset_sum_dev needs                gpbc_subset_sum_workspace_bytes
 */
#ifndef GPBC_BN254_SUBSET_H
#define GPBC_BN254_SUBSET_H
#include "gpbc_bn254.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpbc_subset_table gpbc_subset_table;

int gpbc_subset_version(void);             /* 1 */

/* A table over nbits >= 1 points B_0 .. B_{nbits-1} (gnark G1Affine / G2Affine, taken to be on the curve as gnark's Add takes them; the
 * all-zero point is infinity) and an optional offset point O (Waters' U'; NULL = none): for every byte position w < W = ceil(nbits / 8)
 * and byte value v the subset sum of the eight points of that window — bit 7 - t of byte w selects B_{8w+t}, the reference's bit order
 * and numpy.packbits' default — with O added into window 0, kept in HBM as affine rows of 128 (G1) / 256 (G2) bytes plus one flag byte
 * per row: gpbc_subset_table_bytes(nbits, is_g2) = W x 256 x (129 | 257) bytes, 2 MiB + 8 KiB for Waters05's 256 G2 points.
 * nbits is at most 16384 (2 048 windows: 64.5 MiB in G1, 128.5 MiB in G2); gpbc_subset_table_bytes returns 0 for nbits == 0 or above
 * that.  nbits == 0, nbits > 16384, null bases or a null `out` are GPBC_ERR_INVALID_ARG before any launch or allocation, *out = NULL.
 * The handle is bound to the device it was built on (the calling thread's current device), like gpbc_fixed_base; using it with another
 * device current is GPBC_ERR_INVALID_ARG.  The host forms upload the points, build and wait.  gpbc_subset_table_create_dev takes device
 * pointers, blocks in hipMalloc for the table, enqueues the build (one kernel, one lane per row: at most nine mixed additions and one
 * inversion) on `stream` and returns without waiting: bases and offset must stay valid until that work is done, and the table may be
 * used on the same stream at once — on another stream, or through gpbc_subset_sum (which runs on a stream of the library's own), only
 * after the caller has waited for the build.  gpbc_subset_table_destroy drains the device before it frees; NULL is accepted. */
size_t gpbc_subset_table_bytes(size_t nbits, int is_g2);
int gpbc_g1_subset_table_create(const void *bases, size_t nbits, const void *offset, gpbc_subset_table **out);
int gpbc_g2_subset_table_create(const void *bases, size_t nbits, const void *offset, gpbc_subset_table **out);
int gpbc_subset_table_create_dev(int is_g2, const void *d_bases, size_t nbits, const void *d_offset, void *stream, gpbc_subset_table **out);

/* out[m] = O + sum_{i : bit i of masks row m} B_i for n rows of W bytes each; positions >= nbits in the last byte select nothing,
 * whatever their value.  Outputs are canonical gnark G1Affine / G2Affine (infinity all zero): a group element has one such encoding,
 * so the bytes are those of gpbc_g*_add_batch folded over O and the selected points, doublings and cancellations included.  An item
 * costs one table row and one mixed addition per byte and one conversion to affine; its whole input is its W bytes.
 * n == 0 is a no-op.  A null table, masks or out is GPBC_ERR_INVALID_ARG before any launch, with nothing written.
 * A call whose n alone does not fill the chip cuts the windows into chunks of at least 32 and adds the chunks' partial sums in one more
 * launch: only then (W >= 64 and n < 131072) does the _dev form need a workspace, gpbc_subset_sum_workspace_bytes(t, n) =
 * chunks x n points (0 for one chunk); a short or missing one is GPBC_ERR_INVALID_ARG before any launch.
 * gpbc_subset_sum_dev is ordered on `stream` only, allocates nothing, reads nothing back and does not synchronise.  gpbc_subset_sum
 * stages through the library's own buffers on the calling thread's current device (which must be the table's) and returns with the
 * results on the host; it is not combined across calling threads and not sharded over devices (the table lives on one). */
int gpbc_subset_sum(const gpbc_subset_table *t, const void *masks, size_t n, void *out);
size_t gpbc_subset_sum_workspace_bytes(const gpbc_subset_table *t, size_t n);
int gpbc_subset_sum_dev(const gpbc_subset_table *t, const void *d_masks, size_t n, void *d_out,
                        void *d_workspace, size_t workspace_bytes, void *stream);
int gpbc_subset_table_destroy(gpbc_subset_table *t);

#ifdef __cplusplus
}
#endif
#endif
