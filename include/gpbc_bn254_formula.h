/* LSSS matrices from boolean formulas, entries of libgpbc_bn254.so added after gpbc_bn254_select.h was fixed at gpbc_select_version() 1,
 * beside gpbc_bn254_ext.h, gpbc_bn254_subset.h, gpbc_bn254_hash.h, gpbc_bn254_share.h, gpbc_bn254_indexed.h and gpbc_bn254_recon.h.
 * Everything the main header says about status codes, gpbc_last_error(), devices, host-pointer entries (synchronous) and *_dev entries
 * (device pointers and a `stream`, stream-ordered, not synchronised) holds here; gpbc_formula_version() counts the revisions of this file.
 *
 * A formula is a row of n_nodes int64 codes: the nodes of a binary tree in depth-first preorder (gate, left subtree, right subtree).
 *   code >= 0            a leaf with that attribute, in [0, 2^63)
 *   GPBC_FORMULA_END     padding behind the tree
 *   GPBC_FORMULA_AND     an AND gate
 *   GPBC_FORMULA_OR      an OR gate
 * A row is well formed under this rule: start with need = 1; every node takes 1 from need and a gate adds 2; the tree ends where need
 * reaches 0; every later entry must be END; no earlier entry may be END or below GPBC_FORMULA_OR; a row that ends with need > 0 is
 * malformed.  A row holds at most 127 nodes: 64 leaves, the 64 x 64 limit of gpbc_fr_lsss_shares and gpbc_fr_lsss_weights.
 * Scalars are the ABI's one scalar format: 32 bytes, little-endian, canonical.  Every entry is one kernel launch and needs no workspace.
 *
 * Entry map (what replaces what):
 *   the share matrix (M, rho) of a formula, per item                              gpbc_fr_lsss_from_formula(_dev)
 *       NewLSSSMatrixFromBinaryTree (access/lsss/lewko_waters_lsss_matrix.go:34-87) over And / Or / Leaf
 *       (access/lsss/binary_access_tree_utils.go), in the layout gpbc_fr_lsss_shares and gpbc_fr_lsss_weights read
 *   the rows that recombine with weight 1 for a key, per item                     gpbc_formula_select(_dev)
 *       what FindLinearCombinationWeight solves for in the field; for a matrix made from a formula the weights are 0 and 1
 */
#ifndef GPBC_BN254_FORMULA_H
#define GPBC_BN254_FORMULA_H
#include "gpbc_bn254.h"
#ifdef __cplusplus
extern "C" {
#endif

#define GPBC_FORMULA_END (-1)
#define GPBC_FORMULA_AND (-2)
#define GPBC_FORMULA_OR (-3)
#define GPBC_FORMULA_MAX_NODES 127

int gpbc_formula_version(void);             /* 1 */

/* The Lewko-Waters matrix of k formulas.  nodes: k x n_nodes codes, item-major.  matrix_out: k x rows x cols scalars; rho_out: k x rows
 * int64; dims_out: k x 2 uint32, the item's own row and column count (may be NULL); ok_out: k bytes.
 *   The root has the vector (1); a counter starts at 1.  The nodes are visited in preorder.  An OR gives both children the node's vector.
 *   An AND at counter c gives the left child c zeros followed by -1 (the node's vector is not copied there) and the right child the node's
 *   vector padded with zeros to length c, then 1; the counter becomes c + 1.  A leaf becomes the next row, with its attribute in rho.  At
 *   the end every row is padded with zeros to the counter's value: 1 + the number of AND gates columns, at most one -1 per row.
 *   Entries are 0, 1 or r - 1.  Rows and columns beyond the item's own are zero; rho beyond the item's rows is -1.
 *   ok = 0 for a malformed row, more leaves than `rows` or more columns than `cols`: the item's matrix is all zero, its rho all -1 and its
 *   dims 0, 0.  That is a verdict on the data, not an argument error.
 * 1 <= n_nodes <= 127; 1 <= rows, cols <= 64; k < 2^29; k == 0 is a no-op.  A null pointer other than dims_out, a size out of range, or
 * an output that overlaps the input or another output is GPBC_ERR_INVALID_ARG before any launch, with nothing written.  The host form
 * runs on the calling thread's current device and copies each output straight into the caller's array. */
int gpbc_fr_lsss_from_formula(const int64_t *nodes, size_t n_nodes, size_t k, size_t rows, size_t cols, void *matrix_out, int64_t *rho_out,
                              uint32_t *dims_out, uint8_t *ok_out);
int gpbc_fr_lsss_from_formula_dev(const int64_t *d_nodes, size_t n_nodes, size_t k, size_t rows, size_t cols, void *d_matrix_out,
                                  int64_t *d_rho_out, uint32_t *d_dims_out, uint8_t *d_ok_out, void *stream);

/* The leaves whose rows recombine with weight 1, for k keys.  nodes: n_formulas x n_nodes codes, n_formulas = 1 (one policy for every key)
 * or k; held: k x rows bytes in leaf order, the `held` of gpbc_fr_lsss_weights on the matrix above; chosen_out: k x rows bytes of 0 / 1;
 * ok_out: k bytes.
 *   A leaf is satisfied iff its byte is non-zero, an AND iff both children are, an OR iff either is.  With the root satisfied ok = 1 and
 *   the chosen leaves are those reached from the root by taking both children of an AND and, at an OR, the left child if it is satisfied,
 *   otherwise the right.  Otherwise — an unsatisfied root, a malformed formula, more leaves than `rows` — ok = 0 and the row is zero.
 *   For ok = 1 the chosen rows of the matrix of gpbc_fr_lsss_from_formula sum to (1, 0, ..., 0), and ok equals the ok of
 *   gpbc_fr_lsss_weights on that matrix and mask.
 * 1 <= n_nodes <= 127; 1 <= rows <= 64; k < 2^29; k == 0 is a no-op.  A null pointer, n_formulas other than 1 or k, a size out of range,
 * or an output that overlaps an input or the other output is GPBC_ERR_INVALID_ARG before any launch, with nothing written. */
int gpbc_formula_select(const int64_t *nodes, size_t n_formulas, size_t n_nodes, const uint8_t *held, size_t k, size_t rows,
                        uint8_t *chosen_out, uint8_t *ok_out);
int gpbc_formula_select_dev(const int64_t *d_nodes, size_t n_formulas, size_t n_nodes, const uint8_t *d_held, size_t k, size_t rows,
                            uint8_t *d_chosen_out, uint8_t *d_ok_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
