/* Secret sharing in the scalar field Fr, entries of libgpbc_bn254.so added after the main header (gpbc_bn254.h) was frozen at
 * gpbc_abi_version() 8, beside gpbc_bn254_ext.h, gpbc_bn254_subset.h and gpbc_bn254_hash.h.  Everything the main header says about status
 * codes, gpbc_last_error(), devices, host-pointer entries (synchronous) and *_dev entries (device pointers and a `stream`, stream-ordered,
 * not synchronised) holds here; gpbc_share_version() counts the revisions of this file.
 *
 * Scalars are the ABI's one scalar format: 32 bytes, little-endian.  An input is any value below 2^256 and acts as its residue modulo r;
 * outputs are canonical, in [0, r).  Every entry is one kernel launch and needs no workspace.
 *
 * Entry map (what replaces what):
 *   q(x) for many polynomials and points       gpbc_fr_poly_eval(_dev)
 *       utils.ComputePolynomialValue over the coefficients of utils.GenerateRandomPolynomial, once per attribute of a user in SW05
 *       KeyGenerate (fibe/sw05_fibe_common.go:205-210, fibe/sw05_fibe_large_universe.go:153-167)
 *   the shares of a secret over a threshold tree gpbc_share_tree_create + gpbc_fr_share_tree(_dev)
 *       AccessTreeNode.ShareSecret (access/tree/access_tree_node.go:58-75) under BSW07 Encrypt (cpabe/bsw07/bsw07_cpabe.go:133-170)
 */
#ifndef GPBC_BN254_SHARE_H
#define GPBC_BN254_SHARE_H
#include "gpbc_bn254.h"
#ifdef __cplusplus
extern "C" {
#endif

int gpbc_share_version(void);             /* 1 */

/* out[j][t] = sum_{i < d} coeffs[j][i] * points[j][t]^i modulo r, for k rows j and the m points t of a row.
 *   coeffs: n_coeff_rows x d scalars, lowest degree first; n_coeff_rows is 1 (one polynomial for every row) or k
 *   points: n_point_rows x m scalars; n_point_rows is 1 (one point list for every row) or k
 *   out:    k x m scalars
 * The row conventions are gpbc_fr_lagrange_basis': 1 <= d, m <= 1024 and k < 2^29; anything else, a row count other than 1 or k, a null
 * pointer or an `out` that overlaps an input is GPBC_ERR_INVALID_ARG before any launch, with nothing written.  k == 0 is a no-op.
 * The host form is sharded over the bound devices by rows; a row given once travels whole to every shard. */
int gpbc_fr_poly_eval(const void *coeffs, size_t n_coeff_rows, size_t d, const void *points, size_t n_point_rows, size_t m, size_t k, void *out);
int gpbc_fr_poly_eval_dev(const void *d_coeffs, size_t n_coeff_rows, size_t d, const void *d_points, size_t n_point_rows, size_t m, size_t k,
                          void *d_out, void *stream);

/* A threshold tree as a host array of nodes in depth-first preorder.  Node i is (parent, threshold): parent < i is the index of its parent,
 * GPBC_SHARE_ROOT for node 0 and for node 0 only; threshold == 0 marks a leaf, otherwise the node is a gate and threshold its k of
 * k-of-n.  A node's child position is its rank among the nodes with the same parent, counted from 1 (NewThresholdNode: childIndex = i + 1);
 * leaves are numbered in list order (GenerateLeafID, whose ids start at 1: leaf id y is column y - 1 here); gates are numbered in list order,
 * and gate g owns threshold_g - 1 coefficients, of X^1 .. X^(threshold_g - 1), in that order: the order in which ShareSecret draws them.
 *
 * Limits: at most 1024 leaves, at most 1024 gates, at most 1024 children of one gate.  gpbc_share_tree_create refuses with
 * GPBC_ERR_INVALID_ARG, before the device is touched and with *out = NULL: no nodes, a second root (or none at node 0), parent >= i, a parent
 * that is a leaf, a gate whose threshold exceeds its number of children (so: a gate without children), and anything above the limits.
 * The tree is uploaded once to the calling thread's current device and the handle is bound to it, like gpbc_subset_table; create waits for
 * the upload.  gpbc_share_tree_destroy drains the device before it frees; NULL is accepted. */
typedef struct gpbc_share_tree gpbc_share_tree;
typedef struct { uint32_t parent, threshold; } gpbc_share_node;
#define GPBC_SHARE_ROOT 0xffffffffu
int gpbc_share_tree_create(const gpbc_share_node *nodes, size_t n_nodes, gpbc_share_tree **out);
int gpbc_share_tree_destroy(gpbc_share_tree *t);
size_t gpbc_share_tree_leaves(const gpbc_share_tree *t);      /* L: shares per item; 0 for NULL */
size_t gpbc_share_tree_coeffs(const gpbc_share_tree *t);      /* C: coefficients per item, the sum of threshold - 1 over the gates; 0 for NULL */

/* ShareSecret for k secrets over one tree: a gate with value v and coefficients c_1 .. c_(t-1) has the polynomial
 * q(X) = v + c_1 X + ... + c_(t-1) X^(t-1); the root's value is the item's secret, the child at position x gets q(x), and a leaf's output
 * is its value.  A tree that is a single leaf returns the secret.
 *   secrets: k scalars;  coeffs: k x C scalars, item-major, gate by gate (may be NULL when C == 0);  out: k x L scalars, item-major, leaf order
 * k < 2^29; k == 0 is a no-op.  A null handle, a null pointer, an `out` that overlaps an input, or (for the _dev form and the host form
 * alike) a current device other than the tree's is GPBC_ERR_INVALID_ARG before any launch.  The host form is not sharded (the tree lives
 * on one device). */
int gpbc_fr_share_tree(const gpbc_share_tree *t, const void *secrets, const void *coeffs, size_t k, void *out);
int gpbc_fr_share_tree_dev(const gpbc_share_tree *t, const void *d_secrets, const void *d_coeffs, size_t k, void *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
