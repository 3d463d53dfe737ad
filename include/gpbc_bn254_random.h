/* Seed-addressed randomness on the device, entries of libgpbc_bn254.so added after gpbc_bn254_formula.h was fixed at
 * gpbc_formula_version() 1, beside gpbc_bn254_ext.h, gpbc_bn254_subset.h, gpbc_bn254_hash.h, gpbc_bn254_share.h, gpbc_bn254_indexed.h,
 * gpbc_bn254_recon.h and gpbc_bn254_select.h.  Everything the main header says about status codes, gpbc_last_error(), devices,
 * host-pointer entries (synchronous) and *_dev entries (device pointers and a `hip_stream`, stream-ordered, not synchronised) holds
 * here; gpbc_random_version() counts the revisions of this file.  The ABI is LP64: `stream`, `first` and the counts are 64-bit size_t.
 *
 * block(seed, stream, index) is 64 bytes: the ChaCha20 block function of RFC 8439 section 2.3, 20 rounds, on the state
 *   words 0..3    the constants "expand 32-byte k"
 *   words 4..11   the 32-byte seed as little-endian words
 *   word 12, 13   index, low then high 32 bits (a 64-bit block counter)
 *   word 14, 15   stream, low then high 32 bits (a 64-bit nonce)
 * — original ChaCha20; the indices 0, 1, 2 .. of one stream are a plain ChaCha20 keystream, and RFC 8439's 2.3.2 test vector is the
 * block at index 0x0900000000000001 of stream 0x4a000000.
 * scalar(seed, stream, index) = OS2IP(block) mod r: the 64 bytes as ONE big-endian integer (as fr.Element.SetBytes and hash_to_field
 * read byte strings), reduced — not gnark's mask-and-reject loop: the bias is below 2^-257, every lane does the same work and a
 * scalar's position never depends on earlier draws.  Written in the ABI's one scalar format: 32 bytes, little-endian, canonical.
 *
 * The seed is KEY MATERIAL: whoever holds it can recompute every scalar drawn from it.  `seed` is a HOST pointer to 32 bytes in the
 * host and the _dev forms alike; the bytes travel as kernel arguments, are never staged in a buffer and never appear in
 * gpbc_last_error().
 *
 * Element i of a call uses index first + i (a 64-bit add that carries into word 13).  A null pointer or first + n > 2^64 is
 * GPBC_ERR_INVALID_ARG before any launch, with nothing written; a count of 0 is a no-op whatever the pointers.  Host forms run on the
 * calling thread's current device through the shared staging path; they are not sharded and not combined with other threads' calls.
 * _dev forms enqueue on hip_stream only.  Every entry is one kernel launch and needs no workspace.  Outputs (and d_in) may start at
 * any address; one on a 16-byte boundary is written (read) 128 bits at a time.
 *
 * Entry map (what replaces what):
 *   64-byte blocks of the generator                                                gpbc_random_bytes(_dev)
 *   the scalars an Encrypt / KeyGenerate draws, one per fr.Element.SetRandom()    gpbc_fr_random(_dev)
 *       cpabe/bsw07/bsw07_cpabe.go, utils/generate_random_polynomial.go, fibe/sw05_fibe_common.go:205-210
 *   fr.Element.SetBytes / hash.BytesToField on 64-byte strings                     gpbc_fr_set_bytes64(_dev)
 *       the reduction of gpbc_fr_random on inputs of the caller's choice
 */
#ifndef GPBC_BN254_RANDOM_H
#define GPBC_BN254_RANDOM_H
#include "gpbc_bn254.h"
#ifdef __cplusplus
extern "C" {
#endif

#define GPBC_RANDOM_SEED_BYTES 32
#define GPBC_RANDOM_BLOCK_BYTES 64

int gpbc_random_version(void);              /* 1 */

/* out[64 i .. 64 i + 63] = block(seed, stream, first + i), i < n_blocks */
int gpbc_random_bytes(const void *seed, size_t stream, size_t first, size_t n_blocks, void *out);
int gpbc_random_bytes_dev(const void *seed, size_t stream, size_t first, size_t n_blocks, void *d_out, void *hip_stream);

/* out[i] = scalar(seed, stream, first + i), i < n: n scalars of 32 bytes */
int gpbc_fr_random(const void *seed, size_t stream, size_t first, size_t n, void *out);
int gpbc_fr_random_dev(const void *seed, size_t stream, size_t first, size_t n, void *d_out, void *hip_stream);

/* out[i] = OS2IP(in[64 i .. 64 i + 63]) mod r: hash.BytesToField on 64-byte strings.  An out that overlaps in is
 * GPBC_ERR_INVALID_ARG like a null pointer. */
int gpbc_fr_set_bytes64(const void *in, size_t n, void *out);
int gpbc_fr_set_bytes64_dev(const void *d_in, size_t n, void *d_out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
