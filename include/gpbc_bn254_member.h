/* Membership tests on in-memory elements, entries of libgpbc_bn254.so added after the main header (gpbc_bn254.h) was frozen at
 * gpbc_abi_version() 8, beside the other headers of its kind (gpbc_bn254_ext.h, ..., gpbc_bn254_verify.h).  Everything the main header
 * says about status codes, gpbc_last_error(), devices, host-pointer entries (synchronous) and *_dev entries (device pointers and a
 * `stream`, asynchronous) holds here; gpbc_member_version() counts the revisions of this file.
 *
 * The library takes gnark's in-memory structs unchanged and, elsewhere, trusts them: only an element that arrives in wire format is
 * validated (gpbc_g1/g2_unmarshal_batch check the curve and the G2 subgroup, gpbc_gt_unmarshal_batch the encoding alone).  These entries
 * validate the structs themselves — tensors an earlier kernel left, public keys and signatures other parties contributed.
 *
 * Entry map (what replaces what):
 *   ok[i] = (*G1Affine).IsOnCurve() = (*G1Affine).IsInSubGroup() (cofactor 1)          gpbc_g1_is_on_curve(_dev)
 *   ok[i] = (*G2Affine).IsOnCurve()                                                    gpbc_g2_is_on_curve(_dev)
 *   ok[i] = (*G2Affine).IsInSubGroup(), and on the twist                               gpbc_g2_is_in_subgroup(_dev)
 *   ok[i] = (*GT).IsInSubGroup(), and not zero                                         gpbc_gt_is_in_subgroup(_dev)
 *       the guards of the reference's own tests — signature/zss04_signature/zss04_signature_test.go:62,107,
 *       signature/bb04_signature/bb04_signature_test.go:35-39,98 — and what an aggregator of contributed keys needs before
 *       gka/agka09/asbb.go:193-220 (AggregatePublicKeys sums R_i in G2 and multiplies A_i in GT, AggregateSignatures sums sigma_i in G1).
 *
 * The verdicts (csrc/member29.hip.hpp has the formulas):
 *   every group   a coordinate whose stored 256-bit value — the Montgomery form, as gnark keeps it — is not below p gives 0 before any
 *                 arithmetic: gnark cannot hold such an element.
 *   G1            the point at infinity (0, 0) gives 1, as gnark's IsOnCurve does through its Jacobian form; else y^2 == x^3 + 3.
 *   G2            infinity gives 1; on the twist: y^2 == x^3 + 3 / (9 + i); in the subgroup: on the twist AND
 *                 [x+1]Q + psi([x]Q) + psi^2([x]Q) == psi^3([2x]Q).  gnark's IsInSubGroup evaluates that identity without a curve test of
 *                 its own; the two agree on every point of the twist, and the 0 for a point off the twist is this library's definition.
 *   GT            canonical AND z != 0 AND z^(p^4) z == z^(p^2) AND z^p == z^(6u^2), which on BN254 is z^r == 1 exactly (r = p - 6u^2).
 *                 gnark's E12.IsInSubGroup is the last two; read literally it accepts the ZERO element (both equalities read 0 == 0),
 *                 which this entry rejects on purpose: zero is in no group.
 */
#ifndef GPBC_BN254_MEMBER_H
#define GPBC_BN254_MEMBER_H
#include "gpbc_bn254.h"
#ifdef __cplusplus
extern "C" {
#endif

int gpbc_member_version(void);                                 /* 1 */

/* ok_out[i] = the verdict (1 or 0) for element i of n gnark structs read as they are: G1Affine 64 bytes, G2Affine 128, GT 384.  Nothing
 * but the n verdict bytes is written.  Rows must be 4-byte aligned.  ok_out (n bytes) must not overlap the input.  n == 0 is a no-op; a
 * null pointer with n > 0, a misaligned input, an overlap or n above 2^31 - 1 is GPBC_ERR_INVALID_ARG before any launch, with nothing
 * written.  A *_dev entry is ONE launch, ordered on `stream` only and not synchronised; it allocates nothing and has no workspace.  A
 * host entry stages through the library's device blocks on the calling thread's current device; it is neither sharded over devices nor
 * combined across threads.  The point entries take one point per lane, gpbc_gt_is_in_subgroup one element per lane pair. */
int gpbc_g1_is_on_curve(const void *pts, size_t n, uint8_t *ok_out);
int gpbc_g1_is_on_curve_dev(const void *d_pts, size_t n, uint8_t *d_ok_out, void *stream);
int gpbc_g2_is_on_curve(const void *pts, size_t n, uint8_t *ok_out);
int gpbc_g2_is_on_curve_dev(const void *d_pts, size_t n, uint8_t *d_ok_out, void *stream);
int gpbc_g2_is_in_subgroup(const void *pts, size_t n, uint8_t *ok_out);
int gpbc_g2_is_in_subgroup_dev(const void *d_pts, size_t n, uint8_t *d_ok_out, void *stream);
int gpbc_gt_is_in_subgroup(const void *gt, size_t n, uint8_t *ok_out);
int gpbc_gt_is_in_subgroup_dev(const void *d_gt, size_t n, uint8_t *d_ok_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
