/* Forests of threshold trees in the scalar field Fr: sharing and reconstruction weights with a tree per item, entries of
 * libgpbc_bn254.so added after gpbc_bn254_share.h and gpbc_bn254_recon.h were fixed at version 1, beside gpbc_bn254_ext.h,
 * gpbc_bn254_subset.h, gpbc_bn254_hash.h, gpbc_bn254_indexed.h, gpbc_bn254_select.h, gpbc_bn254_formula.h and gpbc_bn254_random.h.
 * Everything the main header says about status codes, gpbc_last_error(), devices, host-pointer entries (synchronous) and *_dev entries
 * (device pointers and a `stream`, stream-ordered, not synchronised) holds here; gpbc_forest_version() counts the revisions of this file.
 *
 * Scalars are the ABI's one scalar format: 32 bytes, little-endian.  An input is any value below 2^256 and acts as its residue modulo r;
 * outputs are canonical, in [0, r).  Every entry is one kernel launch and needs no workspace.
 *
 * Entry map (what replaces what):
 *   the shares of k secrets, each over a tree of its own        gpbc_share_forest_create + gpbc_fr_share_forest(_dev)
 *       AccessTreeNode.ShareSecret (access/tree/access_tree_node.go:58-75) under BSW07 Encrypt (cpabe/bsw07/bsw07_cpabe.go:133-170), once per
 *       ciphertext with that ciphertext's policy: what gpbc_fr_share_tree does for one policy per call
 *   the weights that recombine them, a tree per item             gpbc_fr_forest_weights(_dev)
 *       AccessTreeNode.DecryptNode (access/tree/access_tree_node.go:96-164) under BSW07 Decrypt (cpabe/bsw07/bsw07_cpabe.go:172-195): what
 *       gpbc_fr_tree_weights does for one policy per call
 */
#ifndef GPBC_BN254_FOREST_H
#define GPBC_BN254_FOREST_H
#include "gpbc_bn254_share.h"
#ifdef __cplusplus
extern "C" {
#endif

int gpbc_forest_version(void);            /* 1 */

/* A forest is n_trees threshold trees, each a node list as gpbc_share_tree_create takes it: tree t is nodes[node_off[t] .. node_off[t + 1]),
 * its parents counted from its own node 0, with the numbering of gpbc_bn254_share.h unchanged (leaf y of a tree is column y - 1; gate g
 * owns threshold_g - 1 coefficients in draw order).  node_off holds n_trees + 1 increasing offsets.  The forest's sizes are the maxima over
 * its trees: Lmax leaves and Cmax coefficients; the per-item arrays of the entries below are padded to them.
 *
 * gpbc_share_forest_create refuses with GPBC_ERR_INVALID_ARG, before the device is touched and with *out = NULL: n_trees == 0,
 * n_trees > 65536, a node_off that does not increase, and any tree gpbc_share_tree_create would refuse — the message names the tree's
 * index and gives that entry's reason.  The forest is uploaded once to the calling thread's current device and the handle is bound to it;
 * create waits for the upload.  gpbc_share_forest_destroy drains the device before it frees; NULL is accepted. */
typedef struct gpbc_share_forest gpbc_share_forest;
int gpbc_share_forest_create(const gpbc_share_node *nodes, const uint32_t *node_off, size_t n_trees, gpbc_share_forest **out);
int gpbc_share_forest_destroy(gpbc_share_forest *f);
size_t gpbc_share_forest_trees(const gpbc_share_forest *f);                   /* T; 0 for NULL */
size_t gpbc_share_forest_leaves(const gpbc_share_forest *f);                  /* Lmax: columns of out, held and w_out; 0 for NULL */
size_t gpbc_share_forest_coeffs(const gpbc_share_forest *f);                  /* Cmax: columns of coeffs; 0 for NULL */
size_t gpbc_share_forest_tree_leaves(const gpbc_share_forest *f, size_t t);   /* L of tree t; 0 for t >= T or NULL */
size_t gpbc_share_forest_tree_coeffs(const gpbc_share_forest *f, size_t t);   /* C of tree t; 0 for t >= T or NULL */

/* ShareSecret for k secrets, item i over tree tree_of[i].
 *   tree_of: k uint32;  secrets: k scalars;  coeffs: k x Cmax scalars, item-major — item i reads its first C_t columns, gate by gate as
 *   gpbc_fr_share_tree reads them, and the rest may hold anything (may be NULL when Cmax == 0);  out: k x Lmax scalars, item-major, the
 *   first L_t columns of item i in its tree's leaf order and the columns >= L_t written as zero;  ok_out: k bytes, 1 where tree_of[i] < T
 *   (may be NULL, in both forms).
 * An item whose tree id is T or more gets an all-zero row and ok = 0; no table is read for it.
 * k < 2^29; k == 0 is a no-op.  A null handle, a null pointer, an output that overlaps an input or the other output, or (for the _dev form
 * and the host form alike) a current device other than the forest's is GPBC_ERR_INVALID_ARG before any launch, with nothing written.
 * The host form is not sharded (the forest lives on one device). */
int gpbc_fr_share_forest(const gpbc_share_forest *f, const uint32_t *tree_of, const void *secrets, const void *coeffs, size_t k, void *out, uint8_t *ok_out);
int gpbc_fr_share_forest_dev(const gpbc_share_forest *f, const uint32_t *d_tree_of, const void *d_secrets, const void *d_coeffs, size_t k, void *d_out, uint8_t *d_ok_out,
                             void *stream);

/* DecryptNode for k attribute sets, item i over tree tree_of[i]: the rules of gpbc_fr_tree_weights on the item's own tree.
 *   held: k x Lmax bytes, item-major; the first L_t columns of item i in its tree's leaf order, a non-zero byte = the leaf is held, and the
 *   columns >= L_t ignored;  w_out: k x Lmax scalars, the columns >= L_t written as zero;  ok_out: k bytes.
 * ok = 0 means "the root is unsatisfied OR the tree id is out of range (tree_of[i] >= T)"; in both cases the item's row is all zero.  A
 * tree that is a single leaf gives 1 when held.  For ok = 1, sum_y w[y] * share[y] = secret modulo r for every output of
 * gpbc_fr_share_forest on the same forest and tree id.
 * k < 2^29; k == 0 is a no-op.  A null handle, a null pointer, outputs that overlap an input or each other, or a current device other than
 * the forest's is GPBC_ERR_INVALID_ARG before any launch, with nothing written.  The host form is not sharded. */
int gpbc_fr_forest_weights(const gpbc_share_forest *f, const uint32_t *tree_of, const uint8_t *held, size_t k, void *w_out, uint8_t *ok_out);
int gpbc_fr_forest_weights_dev(const gpbc_share_forest *f, const uint32_t *d_tree_of, const uint8_t *d_held, size_t k, void *d_w_out, uint8_t *d_ok_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
