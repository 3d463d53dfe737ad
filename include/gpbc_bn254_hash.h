/* SHA-256 on the device with the digest as bytes or as a scalar, entries of libgpbc_bn254.so added after the main header (gpbc_bn254.h)
 * was frozen at gpbc_abi_version() 8, beside the extension header (gpbc_bn254_ext.h, gpbc_ext_version() 2) and the subset header
 * (gpbc_bn254_subset.h, gpbc_subset_version() 1).  Everything the main header says about status codes, gpbc_last_error(), devices,
 * host-pointer entries (synchronous) and *_dev entries (device pointers and a `stream`, asynchronous) holds here; gpbc_hash_version()
 * counts the revisions of this file.
 *
 * Entry map (what replaces what):
 *   beta = H(u, v, w) in Zr, u in G1, v and w in GT                 gpbc_hash_g1_gt_gt_to_fr(_dev)
 *       h() of ibe/gentry06_ibe/gentry06_ibe.go:319-343 — u.Bytes() (:322), v.Bytes() and w.Bytes() (:323-324) concatenated, SHA-256,
 *       fr.Element.SetBytes — which Encrypt calls between u, v, w and y (:226) and Decrypt before anything is paired (:266): with this
 *       entry neither the 800 bytes nor beta leave the device
 *   SHA-256 of a byte string, as 32 bytes                           gpbc_sha256_batch(_dev), to_fr = 0
 *       NewWaters05IBEIdentity (ibe/waters05_ibe/waters05_ibe.go:290-315: the digest's 256 bits are Id[], and as rows of 32 bytes the
 *       masks of gpbc_subset_sum) and NewBB04IBEIdentity, one digest per identity
 *   SHA-256 of a byte string, as a scalar                           gpbc_sha256_batch(_dev), to_fr = 1
 *       fr.Element.SetBytes(sha256.Sum256(m)): the digest as a big-endian integer, reduced mod r
 */
#ifndef GPBC_BN254_HASH_H
#define GPBC_BN254_HASH_H
#include "gpbc_bn254.h"
#ifdef __cplusplus
extern "C" {
#endif

int gpbc_hash_version(void);                                   /* 1 */

/* SHA-256 of n messages, one per lane.  Message i is msgs[msg_off[i], msg_off[i+1]): msg_off holds n + 1 offsets into msgs, as the
 * hash-to-curve entries take them.  The host form refuses decreasing offsets (GPBC_ERR_INVALID_ARG); the _dev form is given
 * msgs_bytes, the length of the message buffer, and clamps every offset to [0, msgs_bytes] and every message to a length >= 0, so a
 * malformed device-resident table cannot make the kernel read outside the buffer.  A null msgs is accepted when no message has a byte.
 * out: n rows of 32 bytes.  to_fr == 0: the digest as SHA-256 writes it.  to_fr != 0: that digest read as a big-endian integer and
 * reduced mod r, in the ABI's one scalar format (32 bytes, little-endian, canonical in [0, r)) — directly usable as `scalars` of every
 * multiplication / exponentiation / Fr entry.
 * n == 0 is a no-op.  A null msg_off or out (or msgs, where a message has bytes) with n > 0 is GPBC_ERR_INVALID_ARG before any launch,
 * with nothing written.  gpbc_sha256_batch_dev is ordered on `stream` only, allocates nothing, reads nothing back and does not
 * synchronise.  gpbc_sha256_batch stages through the library's own device blocks on the calling thread's current device and returns
 * with the results on the host; it is not combined across calling threads and not sharded over devices. */
int gpbc_sha256_batch(const void *msgs, const uint64_t *msg_off, size_t n, int to_fr, void *out);
int gpbc_sha256_batch_dev(const void *d_msgs, const uint64_t *d_msg_off, size_t msgs_bytes, size_t n, int to_fr,
                          void *d_out, void *stream);

/* out[i] = fr.SetBytes(SHA-256(u[i].Bytes() || v[i].Bytes() || w[i].Bytes())) for n items, one per lane.  u: n gnark G1Affine structs
 * (64 B); v, w: n gnark GT structs (384 B); out: n scalars in the ABI's one scalar format, canonical.  The hashed stream is the 800
 * bytes gpbc_g1_marshal_batch(compressed) and gpbc_gt_marshal_batch write: u.X big-endian with the form in its two top bits (0x80 / 0xC0
 * by the sign of Y; the all-zero u is infinity and hashes as 0x40 and 31 zero bytes), then the twelve coefficients of v and of w from
 * C1.B2.A1 down to C0.B0.A0.  GT elements are encoded as they are: there is no membership test, zero and one are ordinary inputs.
 * n == 0 is a no-op.  A null pointer with n > 0 is GPBC_ERR_INVALID_ARG before any launch, with nothing written.  The _dev form is one
 * launch, ordered on `stream` only; it allocates nothing, reads nothing back and does not synchronise.  The host form stages through
 * the library's own device blocks on the calling thread's current device and returns with the results on the host; it is not combined
 * across calling threads and not sharded over devices. */
int gpbc_hash_g1_gt_gt_to_fr(const void *u, const void *v, const void *w, size_t n, void *out);
int gpbc_hash_g1_gt_gt_to_fr_dev(const void *d_u, const void *d_v, const void *d_w, size_t n, void *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
