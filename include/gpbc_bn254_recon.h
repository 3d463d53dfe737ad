/* Reconstruction weights of a threshold tree in the scalar field Fr, entries of libgpbc_bn254.so added after gpbc_bn254_share.h was
 * fixed at gpbc_share_version() 1, beside gpbc_bn254_ext.h, gpbc_bn254_subset.h, gpbc_bn254_hash.h and gpbc_bn254_indexed.h.  Everything
 * the main header says about status codes, gpbc_last_error(), devices, host-pointer entries (synchronous) and *_dev entries (device
 * pointers and a `stream`, stream-ordered, not synchronised) holds here; gpbc_recon_version() counts the revisions of this file.
 *
 * Scalars are the ABI's one scalar format: 32 bytes, little-endian; outputs are canonical, in [0, r).  Every entry is one kernel launch
 * and needs no workspace.  The tree is the handle of gpbc_bn254_share.h: gpbc_share_tree_create uploads what both directions need.
 *
 * Entry map (what replaces what):
 *   the weights that recombine the shares of a threshold tree   gpbc_fr_tree_weights(_dev)
 *       AccessTreeNode.DecryptNode (access/tree/access_tree_node.go:96-164) under BSW07 Decrypt (cpabe/bsw07/bsw07_cpabe.go:172-195): the
 *       walk that finds the satisfied children of every gate, and the Lagrange coefficients (utils/compute_lagrange_basis.go:8-30) it
 *       applies gate by gate as GT exponents, here multiplied down each leaf's path into one scalar per leaf
 */
#ifndef GPBC_BN254_RECON_H
#define GPBC_BN254_RECON_H
#include "gpbc_bn254_share.h"
#ifdef __cplusplus
extern "C" {
#endif

int gpbc_recon_version(void);             /* 1 */

/* DecryptNode for k attribute sets over one tree.  held: k x L bytes, item-major, leaf order (the columns of gpbc_fr_share_tree's output);
 * a non-zero byte means the item holds the leaf's attribute.  w_out: k x L scalars; ok_out: k bytes.
 *   A leaf is satisfied iff it is held, a gate iff at least `threshold` of its children are.  A satisfied gate uses its first `threshold`
 *   satisfied children in child order, at positions S (counted from 1); the used child at position i takes the factor
 *   Delta_{i,S}(0) = prod_{j in S, j != i} (0 - j) / (i - j) modulo r.  The weight of a used leaf is the product of the factors on its path
 *   from the root; every other leaf — not held, or held under a gate that is unsatisfied or not among the chosen — gets 0.
 *   ok = 1 iff the root is satisfied; otherwise ok = 0 and the item's row is all zero.  A tree that is a single leaf gives 1 when held.
 * For ok = 1, sum_y w[y] * share[y] = secret modulo r for every output of gpbc_fr_share_tree on the same tree.
 * k < 2^29; k == 0 is a no-op.  A null handle, a null pointer, outputs that overlap the input or each other, or (for the _dev form and the
 * host form alike) a current device other than the tree's is GPBC_ERR_INVALID_ARG before any launch, with nothing written.  The host
 * form is not sharded (the tree lives on one device). */
int gpbc_fr_tree_weights(const gpbc_share_tree *t, const uint8_t *held, size_t k, void *w_out, uint8_t *ok_out);
int gpbc_fr_tree_weights_dev(const gpbc_share_tree *t, const uint8_t *d_held, size_t k, void *d_w_out, uint8_t *d_ok_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
