// Membership tests on IN-MEMORY elements (include/gpbc_bn254_member.h): gnark's (*G1Affine).IsOnCurve / IsInSubGroup,
// (*G2Affine).IsOnCurve / IsInSubGroup and (*GT).IsInSubGroup as verdicts, for structs that did not come through Unmarshal — tensors an
// earlier kernel left, keys and signatures other parties contributed (the reference's tests guard those: signature/zss04_signature/
// zss04_signature_test.go:62,107, signature/bb04_signature/bb04_signature_test.go:35-39,98; gka/agka09/asbb.go:193-220 aggregates them).
//
// One rule for the three groups: a coordinate whose stored 256-bit value (the Montgomery form, as gnark keeps it) is not below p is not a
// representation gnark can hold; the verdict is 0, decided on the words before any arithmetic.  Such a coordinate then enters the
// arithmetic as zero, so that every value stays in the interval classes the field code is proved for (GPBC_BOUNDS) — the verdict is
// already fixed and what is computed from it is thrown away.
//
//   G1  infinity (0, 0) -> 1 (gnark's IsOnCurve answers through the Jacobian form, where infinity is on the curve); else y^2 == x^3 + 3.
//       IsInSubGroup is the same verdict (cofactor 1).
//   G2  infinity -> 1; on the twist: y^2 == x^3 + 3 / (9 + i); in the subgroup: on the twist AND g2_in_subgroup29 (wire29.hip.hpp),
//       the endomorphism identity [x+1]Q + psi([x]Q) + psi^2([x]Q) == psi^3([2x]Q).  gnark's IsInSubGroup evaluates the identity alone,
//       without a curve test; the two agree on every point of the twist, and rejecting a point off the twist is THIS project's
//       definition (parity unpinned) — the group law used by the identity means nothing off the twist.
//   GT  one element per lane pair (tower29_pair.hip.hpp).  The verdict is the conjunction of
//         canonical coordinates;  z != 0;  z^(p^4) z == z^(p^2) (f12p_is_cyclotomic);  z^p == z^(6 u^2)
//       — the last two are gnark's E12.IsInSubGroup, and on BN254 z^p == z^(6u^2) is z^r == 1 exactly, since r = p - 6u^2.
//       z^(6u^2): t = expt(expt(z)) (f12p_expt_to, the x^u chain of the final exponentiation), two Granger-Scott squarings for t^2 and
//       t^4, one product for t^6.
//       ZERO: a literal reading of gnark's two equalities accepts the zero element (both read 0 == 0).  It is in no group; this entry
//       rejects it on purpose.
//       A lane pair that failed an earlier test still runs the chain beside its neighbours (no divergence inside the DPP exchanges);
//       its Granger-Scott squarings then work on meaningless values, which only have to stay inside the limb bounds — the interval
//       classes do not depend on the subgroup, and tools/bounds_check.cpp (hc_gt_is_in_subgroup with force = 1) runs such elements
//       through the whole chain.  Only a wavefront in which NO lane pair is still a candidate skips the chain (X::all: one ballot, a
//       uniform branch); every verdict there is 0 already.
#ifndef GPBC_MEMBER29_HIP_HPP
#define GPBC_MEMBER29_HIP_HPP
#include "wire29.hip.hpp"
#include "pairing29_pair.hip.hpp"

namespace gpbc {

// One stored coordinate: false when its 256-bit value is not below p (the coordinate is then loaded as zero); `zero`: all words zero.
GPBC_INLINE bool member_fe_load(Fe &r, const uint8_t *p, bool &zero) {
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = q[i];
    zero = wire_words_zero(w);
    const bool canonical = wire_words_canonical(w);
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = canonical ? w[i] : 0u;
    r = fe_from_words(w);
    return canonical;
}
GPBC_INLINE bool member_f2_load(F2 &r, const uint8_t *p, bool &zero) {
    bool z0, z1;
    const bool c0 = member_fe_load(r.a0, p, z0), c1 = member_fe_load(r.a1, p + 32, z1);
    zero = z0 && z1;
    return c0 && c1;
}

// (*G1Affine).IsOnCurve on the 64 bytes at p
GPBC_INLINE bool g1_member_on_curve(const uint8_t *p) {
    Fe x, y;
    bool zx, zy;
    const bool cx = member_fe_load(x, p, zx), cy = member_fe_load(y, p + 32, zy);
    if (!(cx && cy)) return false;
    if (zx && zy) return true;
    constexpr int32_t B3[NL] = F29_B_G1;
    return g_equal(fe_sqr(y), fe_norm(fe_add(fe_mul(fe_sqr(x), x), fe_const(B3))));
}
// (*G2Affine).IsOnCurve (subgroup = false) and IsInSubGroup on the 128 bytes at p
GPBC_INLINE bool g2_member(const uint8_t *p, bool subgroup) {
    F2 x, y;
    bool zx, zy;
    const bool cx = member_f2_load(x, p, zx), cy = member_f2_load(y, p + 64, zy);
    if (!(cx && cy)) return false;
    if (zx && zy) return true;
    constexpr int32_t BT[2][NL] = F29_B_G2;
    if (!g_equal(f2_sqr(y), f2_norm(f2_add(f2_mul(f2_sqr(x), x), f2_const(BT))))) return false;
    return !subgroup || g2_in_subgroup29(x, y);
}

// the same verdict on both lanes of a pair from each lane's own
template <class X> GPBC_INLINE bool member_pair_and(const X &x, bool mine) {
    const Fe flag = x.swap(fe_sel(mine, fe_one(), fe_zero()));
    return mine && !fe_is_zero(flag);
}
// (*GT).IsInSubGroup for the lane pair's element; `half` points at this lane's 192 bytes (even lane C0, odd lane C1).  force: run the
// chain whatever the earlier tests said (the host harness's proof of the limb bounds; the kernel passes false).
template <class X> GPBC_INLINE bool gt_member_pair(const X &x, const uint8_t *half, bool force) {
    F6 z;
    bool zb0, zb1, zb2;
    const bool c0 = member_f2_load(z.b0, half, zb0), c1 = member_f2_load(z.b1, half + 64, zb1), c2 = member_f2_load(z.b2, half + 128, zb2);
    const bool canonical = member_pair_and(x, c0 && c1 && c2);
    const bool zero = member_pair_and(x, zb0 && zb1 && zb2);
    bool candidate = canonical && !zero;
    candidate = f12p_is_cyclotomic(x, z) && candidate;            // every lane pair: the test holds DPP exchanges
    if (!force && x.all(!candidate)) return false;                // nothing left to decide in this wavefront
    F6 t, t2, t4;
    f12p_expt_to(x, t, z);
    f12p_expt_to(x, t2, t);                                       // z^(u^2)
    t2 = f12p_cyclo_sqr<true>(x, t2);
    t4 = f12p_cyclo_sqr<true>(x, t2);
    f12p_mul_to(x, t, t2, t4);                                    // z^(6 u^2)
    const F6 d = f6_norm(f6_sub(t, f12p_frob(x, z, 1)));
    const bool mine = f2_is_zero(d.b0) && f2_is_zero(d.b1) && f2_is_zero(d.b2);
    return member_pair_and(x, mine) && candidate;
}

}  // namespace gpbc
#endif
