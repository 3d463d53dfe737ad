/* The XOR mask from GT bytes, entries of libgpbc_bn254.so added after the main header (gpbc_bn254.h) was frozen at gpbc_abi_version() 8,
 * beside the other headers of its kind (gpbc_bn254_ext.h, gpbc_bn254_subset.h, gpbc_bn254_hash.h, ...).  Everything the main header says
 * about status codes, gpbc_last_error(), devices, host-pointer entries (synchronous) and *_dev entries (device pointers and a `stream`,
 * asynchronous) holds here; gpbc_mask_version() counts the revisions of this file.
 *
 * Entry map (what replaces what):
 *   C2 = M xor H2(gid), M = C2 xor H2(gid), gid in GT, M and C2 byte strings        gpbc_gt_xor_mask(_dev)
 *       utils.Xor(message.Message, hash.FromGT(gid)), the last step of Encrypt (ibe/bf01_ibe/bf01_ibe.go:170-176), and
 *       utils.Xor(ciphertext.C2, hash.FromGT(gid)), the last step of Decrypt (:202-208), of Boneh-Franklin BasicIdent.
 *       hash.FromGT is GT.Bytes() (hash/hash_from_gt.go:5-8): 384 bytes, the twelve coefficients as big-endian canonical integers from
 *       C1.B2.A1 down to C0.B0.A0 — what gpbc_gt_marshal_batch writes.  utils.Xor (utils/xor.go:3-16) returns a slice of the SHORTER
 *       operand's length: a message longer than 384 bytes is cut, which is the reference's behaviour and is kept.  With this entry
 *       neither the 384 bytes nor a per-item length leave the device, messages of different lengths go in one launch, and only the
 *       coefficients a message reaches are converted out of Montgomery form.
 */
#ifndef GPBC_BN254_MASK_H
#define GPBC_BN254_MASK_H
#include "gpbc_bn254.h"
#ifdef __cplusplus
extern "C" {
#endif

int gpbc_mask_version(void);                                   /* 1 */

/* For n items, with B_i = GT.Bytes() of gt[i] (384 bytes), len_i the length of message i and L_i = min(len_i, 384):
 *     out_i[j] = msg_i[j] ^ B_i[j]   for 0 <= j < L_i          out_i[j] = 0   for L_i <= j < len_i          out_len[i] = L_i
 * out_len[i] is the length of the slice utils.Xor returns; the bytes past it are zeroed so that the output buffer is fully defined.
 * gt: n gnark GT structs (384 B each), encoded as they are: no membership test, zero and one are ordinary inputs.
 * msg_off != NULL: message i is msgs[msg_off[i], msg_off[i+1]) — n + 1 offsets into msgs, as gpbc_sha256_batch takes them — and `width`
 * is ignored.  msg_off == NULL: the messages are n rows of `width` bytes; any width >= 0 is allowed, a width above 384 gives zero tails.
 * out has the layout of msgs and is written through the same offsets; bytes of out that belong to no message are not touched.
 * out_len: n uint32, or NULL when it is not wanted.  Messages may start at any address and have any length, 0 included.
 * out == msgs (the identical pointer) runs in place.  gt overlapping out is refused, and so is, in the host form, any other overlap of
 * out and msgs (GPBC_ERR_INVALID_ARG).  The host form refuses decreasing offsets (GPBC_ERR_INVALID_ARG); the _dev form is given
 * msgs_bytes, the length of the message buffer (and of out), clamps every offset to [0, msgs_bytes] and every message to a length >= 0,
 * so a malformed device-resident table cannot make the kernel read or write outside the buffers, and in row mode requires
 * n * width <= msgs_bytes.
 * n == 0 is a no-op.  A null gt, or a null msgs or out where some message has a byte (_dev: where msgs_bytes, in row mode n * width, is
 * not 0), with n > 0 is GPBC_ERR_INVALID_ARG before any launch, with nothing written.  gpbc_gt_xor_mask_dev is ONE launch, ordered on
 * `stream` only; it allocates nothing, reads nothing back and does not synchronise.  gpbc_gt_xor_mask stages through the library's own
 * device blocks on the calling thread's current device and returns with the results on the host; it is not combined across calling
 * threads and not sharded over devices. */
int gpbc_gt_xor_mask(const void *gt, const void *msgs, const uint64_t *msg_off, size_t width, size_t n,
                     void *out, uint32_t *out_len);
int gpbc_gt_xor_mask_dev(const void *d_gt, const void *d_msgs, const uint64_t *d_msg_off, size_t msgs_bytes, size_t width,
                         size_t n, void *d_out, uint32_t *d_out_len, void *stream);

#ifdef __cplusplus
}
#endif
#endif
