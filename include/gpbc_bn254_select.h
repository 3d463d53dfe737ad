/* The common attributes of a list and a set in the scalar field Fr, entries of libgpbc_bn254.so added after gpbc_bn254_recon.h was fixed
 * at gpbc_recon_version() 1, beside gpbc_bn254_ext.h, gpbc_bn254_subset.h, gpbc_bn254_hash.h, gpbc_bn254_share.h and gpbc_bn254_indexed.h.
 * Everything the main header says about status codes, gpbc_last_error(), devices, host-pointer entries (synchronous) and *_dev entries
 * (device pointers and a `stream`, stream-ordered, not synchronised) holds here; gpbc_select_version() counts the revisions of this file.
 *
 * Scalars are the ABI's one scalar format: 32 bytes, little-endian.  Inputs may be any value below 2^256 and are compared as field
 * elements (modulo r, as the keys of a map of fr.Element are); the values that come out are canonical, in [0, r).  Every entry is one
 * kernel launch and needs no workspace.
 *
 * Entry map (what replaces what):
 *   the first d distinct attributes of a ciphertext that a key holds, per item   gpbc_fr_find_common(_dev)
 *       utils.FindCommonAttributes (utils/find_common_attributes.go:7-35) as SW05 Decrypt calls it per ciphertext
 *       (fibe/sw05_fibe_common.go:284-333, and the large universe's Decrypt), with the positions of the kept attributes in both lists,
 *       which the reference finds again by value in its loop over the common attributes
 */
#ifndef GPBC_BN254_SELECT_H
#define GPBC_BN254_SELECT_H
#include "gpbc_bn254.h"
#ifdef __cplusplus
extern "C" {
#endif

int gpbc_select_version(void);             /* 1 */

/* FindCommonAttributes(set, list, d) for k items.  sets: n_sets x m scalars, n_sets = 1 (one set for every item) or k (item-major);
 * lists: k x a scalars, item-major.  set_pos_out, list_pos_out: k x d uint32 each; common_out: k x d scalars; ok_out: k bytes.
 *   The list is walked in order.  An element is kept iff the set holds an element equal to it modulo r and no earlier list element equal
 *   to it modulo r was kept; the walk stops after d kept elements.  Slot s of an item's rows describes the s-th kept element: its position
 *   in the set (the FIRST set element equal to it), its position in the list, and its value, canonical — the row of values is the node set
 *   gpbc_fr_lagrange_basis takes as it is.
 *   ok = 1 iff d elements were kept; otherwise ok = 0 and the item's three rows are all zero.  d > min(a, m) is valid and gives ok = 0.
 * 1 <= m, a, d <= 1024; k < 2^29; k == 0 is a no-op.  A null pointer, n_sets other than 1 or k, a size out of range, or an output that
 * overlaps an input or another output is GPBC_ERR_INVALID_ARG before any launch, with nothing written.  The host form is sharded over the
 * bound devices like gpbc_fr_lsss_weights; a set given once travels whole to every shard. */
int gpbc_fr_find_common(const void *sets, size_t n_sets, size_t m, const void *lists, size_t a, size_t d, size_t k, uint32_t *set_pos_out,
                        uint32_t *list_pos_out, void *common_out, uint8_t *ok_out);
int gpbc_fr_find_common_dev(const void *d_sets, size_t n_sets, size_t m, const void *d_lists, size_t a, size_t d, size_t k,
                            uint32_t *d_set_pos_out, uint32_t *d_list_pos_out, void *d_common_out, uint8_t *d_ok_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
