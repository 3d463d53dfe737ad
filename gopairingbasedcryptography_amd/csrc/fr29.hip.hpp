// BN254 scalar field Fr (integers modulo the group order r) for gfx950, in the shape of fe29.hip.hpp: nine SIGNED 29-bit limbs,
// Montgomery radix R' = 2^261, lazy reduction, one v_mad_i64_i32 per limb pair.  Replaces gnark-crypto's fr.Element arithmetic
// where the reference does it per item of a batch: the quotient polynomials of bibe/afp25_bibe (afp25_bibe_utils.go:14-55) and
// bibe/gwww25_bibe, the exponent 1 / (H(m) + x) of signature/zss04_signature/zss04_signature.go:249-252 and
// signature/bb04_signature/bb04_signature.go:233, key extraction in ibe/gentry06_ibe/gentry06_ibe.go:151.
//
// A header of its own: fe29.hip.hpp and everything built on it stay as they are.  What it takes from there is modulus-free: the limb
// geometry (NL, LB, LMASK), the carry-free linear operations on limb vectors, the safegcd divsteps and the interval harness.  The
// harness measures values in units of p and top limbs with P_OVER_2_232 = ceil(p / 2^232), products with P_OVER_RP >= p / 2^261;
// r < p and the two agree in bits 253..128 (tools/gen_constants.py asserts it), so read in units of r the same constants are valid
// UPPER bounds: |value| <= vb r <= vb p.  Every product asserts its int64 columns under -DGPBC_BOUNDS exactly like fe_mul.
//
// External format = the ABI's one scalar format: 32 bytes, little-endian, plain integer.  Inputs may be any value below 2^256 and act
// as their residue; outputs are canonical in [0, r).  A value is held either "plain" (the limbs are the integer, possibly lazily
// reduced) or "internal" (x 2^261 mod r); mont(a, b) = a b / 2^261, so a plain and an internal factor give a plain product — the
// kernels below convert only what they multiply by many times (a root), never the data they stream.
#ifndef GPBC_FR29_HIP_HPP
#define GPBC_FR29_HIP_HPP
#include "fe29.hip.hpp"

namespace gpbc {

// `l`: limbs and (harness) two-sided bounds in units of r.  `lob`: one-sided knowledge the canonical form needs — value >= -lob r.
struct Fr {
    Fe l;
#ifdef GPBC_BOUNDS
    double lob;
#endif
};

GPBC_INLINE constexpr int32_t fr29_r(int i) { constexpr int32_t M[NL] = FR29_R; return M[i]; }

GPBC_INLINE Fr fr_const(const int32_t (&c)[NL]) { Fr r; r.l = fe_const(c); GPBC_B(r.lob = 0;) return r; }   // a value in [0, r)
GPBC_INLINE Fr fr_zero() { Fr r; r.l = fe_zero(); GPBC_B(r.lob = 0;) return r; }
GPBC_INLINE Fr fr_one() { constexpr int32_t C[NL] = FR29_ONE; return fr_const(C); }                 // internal 1
GPBC_INLINE Fr fr_plain_one() { constexpr int32_t C[NL] = F29_PLAIN_ONE; return fr_const(C); }      // the integer 1

// carry-free linear operations: the limb arithmetic of fe_add / fe_sub / fe_neg / fe_norm knows no modulus
GPBC_INLINE Fr fr_add(const Fr &a, const Fr &b) { Fr r; r.l = fe_add(a.l, b.l); GPBC_B(r.lob = a.lob + b.lob;) return r; }
GPBC_INLINE Fr fr_sub(const Fr &a, const Fr &b) { Fr r; r.l = fe_sub(a.l, b.l); GPBC_B(r.lob = a.lob + b.l.vb;) return r; }
GPBC_INLINE Fr fr_neg(const Fr &a) { Fr r; r.l = fe_neg(a.l); GPBC_B(r.lob = a.l.vb;) return r; }
GPBC_INLINE Fr fr_norm(const Fr &a) { Fr r; r.l = fe_norm(a.l); GPBC_B(r.lob = a.lob;) return r; }

// (a b [+ c d]) / 2^261 mod r: fe_mul_core's column-wise Montgomery product with the modulus r.
// Output: limbs 0..7 in [0, 2^29), limb 8 signed and small; value in (-eps r, (1 + eps) r), eps = (|a b| + |c d|) / (2^261 r).
template <bool TWO>
GPBC_INLINE Fr fr_mul_core(const Fr &A, const Fr &B, const Fr &C, const Fr &D) {
    const Fe &a = A.l, &b = B.l, &c = C.l, &d = D.l;
#ifdef GPBC_BOUNDS
    for (int k = 0; k < 2 * NL - 1; k++) {
        double sl = 0, sh = 0;
        for (int i = 0; i < NL; i++) {
            int j = k - i;
            if (j < 0 || j >= NL) continue;
            double pl, ph;
            prod_interval(a.lo[i], a.hi[i], b.lo[j], b.hi[j], pl, ph); sl += pl; sh += ph;
            if (TWO) { prod_interval(c.lo[i], c.hi[i], d.lo[j], d.hi[j], pl, ph); sl += pl; sh += ph; }
        }
        check_columns(sl, sh, "fr_mul column");
    }
    bound_stats().muls++;
    if (TWO) bound_stats().muls2++;
    bound_stats().mads += (TWO ? 2 : 1) * NL * NL + NL * NL;
#endif
    int32_t m[NL];
    Fr r;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 2 * NL - 1; k++) {
#pragma unroll
        for (int i = 0; i < NL; i++) {
            const int j = k - i;
            if (j < 0 || j >= NL) continue;
            acc += (int64_t)a.v[i] * (int64_t)b.v[j];
            if (TWO) acc += (int64_t)c.v[i] * (int64_t)d.v[j];
        }
#pragma unroll
        for (int i = 0; i < NL; i++) {
            const int j = k - i;
            if (j < 1 || j >= NL) continue;
            acc += (int64_t)m[i] * (int64_t)fr29_r(j);
        }
        if (k < NL) {
            m[k] = (int32_t)(((uint32_t)acc * (uint32_t)FR29_RINV) & (uint32_t)LMASK);
            acc += (int64_t)m[k] * (int64_t)fr29_r(0);
        } else {
            r.l.v[k - NL] = (int32_t)(acc & LMASK);
        }
        acc >>= LB;
    }
    r.l.v[NL - 1] = (int32_t)acc;
#ifdef GPBC_BOUNDS
    const double eps = (a.vb * b.vb + (TWO ? c.vb * d.vb : 0.0)) * P_OVER_RP;     // r / 2^261 < P_OVER_RP
    set_class_n(r.l, eps + 1.0);
    r.lob = eps;
    if (r.l.hi[NL - 1] >= 268435456.0) bounds_fail("fr_mul output top limb", r.l.hi[NL - 1], 268435456.0);
    check_limbs(r.l, "fr_mul output");
#endif
    return r;
}
#if defined(__HIP_DEVICE_COMPILE__) && !defined(GPBC_BOUNDS)
// leaf functions, every limb a scalar argument (fe_mul_leaf's reason: the multipliers exist once in the code object)
__device__ __noinline__ Fe fr_mul_leaf(GPBC_ARGS9(a), GPBC_ARGS9(b)) {
    Fr a, b; a.l = GPBC_PACK9(a); b.l = GPBC_PACK9(b);
    return fr_mul_core<false>(a, b, a, b).l;
}
__device__ __noinline__ Fe fr_mul2_leaf(GPBC_ARGS9(a), GPBC_ARGS9(b), GPBC_ARGS9(c), GPBC_ARGS9(d)) {
    Fr a, b, c, d; a.l = GPBC_PACK9(a); b.l = GPBC_PACK9(b); c.l = GPBC_PACK9(c); d.l = GPBC_PACK9(d);
    return fr_mul_core<true>(a, b, c, d).l;
}
GPBC_INLINE Fr fr_mul(const Fr &a, const Fr &b) { Fr r; r.l = fr_mul_leaf(GPBC_PASS9(a.l), GPBC_PASS9(b.l)); return r; }
GPBC_INLINE Fr fr_mul2(const Fr &a, const Fr &b, const Fr &c, const Fr &d) {
    Fr r; r.l = fr_mul2_leaf(GPBC_PASS9(a.l), GPBC_PASS9(b.l), GPBC_PASS9(c.l), GPBC_PASS9(d.l)); return r;
}
#else
GPBC_INLINE Fr fr_mul(const Fr &a, const Fr &b) { return fr_mul_core<false>(a, b, a, b); }
GPBC_INLINE Fr fr_mul2(const Fr &a, const Fr &b, const Fr &c, const Fr &d) { return fr_mul_core<true>(a, b, c, d); }
#endif
GPBC_INLINE Fr fr_sqr(const Fr &a) { return fr_mul(a, a); }
// the two-product form expanded in place: for a kernel whose one hot loop is this product (the leaf takes 36 limbs, four of them
// through the stack)
GPBC_INLINE Fr fr_mul2_inline(const Fr &a, const Fr &b, const Fr &c, const Fr &d) { return fr_mul_core<true>(a, b, c, d); }

// [0, r), limbs in [0, 2^29) (limb 8 below 2^22), from a value in [-ADD r, (REPS + 1 - ADD) r): add ADD r while the carries are
// propagated, then subtract r while that leaves no borrow, REPS times.  A product (fr_mul) needs <1, 2>.
template <int ADD, int REPS>
GPBC_INLINE Fr fr_canonical(const Fr &a) {
    int32_t t[NL];
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < NL - 1; i++) { int64_t s = (int64_t)a.l.v[i] + ADD * (int64_t)fr29_r(i) + c; t[i] = (int32_t)(s & LMASK); c = s >> LB; }
    t[NL - 1] = (int32_t)((int64_t)a.l.v[NL - 1] + ADD * (int64_t)fr29_r(NL - 1) + c);
#pragma unroll
    for (int rep = 0; rep < REPS; rep++) {
        int32_t d[NL];
        int32_t b = 0;
#pragma unroll
        for (int i = 0; i < NL - 1; i++) { int32_t s = t[i] - fr29_r(i) + b; d[i] = s & LMASK; b = s >> LB; }
        d[NL - 1] = t[NL - 1] - fr29_r(NL - 1) + b;
        const bool ge = d[NL - 1] >= 0;
#pragma unroll
        for (int i = 0; i < NL; i++) t[i] = ge ? d[i] : t[i];
    }
    Fr r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.l.v[i] = t[i];
#ifdef GPBC_BOUNDS
    if (a.lob > (double)ADD) bounds_fail("fr_canonical input below -ADD r", a.lob, (double)ADD);
    if (a.l.vb + ADD >= REPS + 1.0) bounds_fail("fr_canonical input above (REPS + 1 - ADD) r", a.l.vb + ADD, REPS + 1.0);
    set_class_n(r.l, 1.0);
    r.lob = 0;
#endif
    return r;
}
GPBC_INLINE bool fr_limbs_zero(const Fr &c) {        // of a canonical value
    int32_t o = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) o |= c.l.v[i];
    return o == 0;
}

// ------------------------------------------------------------------------------------------------ scalar format <-> limbs
// the 32 bytes as they are: any integer below 2^256 < 5.3 r as a plain value (limbs 0..7 in [0, 2^29), limb 8 below 2^24)
GPBC_INLINE Fr fr_load_raw(const uint8_t *p) {
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = q[i];
    Fr x;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        int bit = LB * i, wi = bit >> 5, sh = bit & 31;
        uint64_t two = (uint64_t)w[wi] | ((wi + 1 < 8) ? ((uint64_t)w[wi + 1] << 32) : 0);
        x.l.v[i] = (int32_t)((two >> sh) & (uint64_t)LMASK);
    }
    GPBC_B(set_class_n(x.l, 5.3); x.l.lo[NL - 1] = 0; x.lob = 0;)        // 2^256 / r = 5.29; 5.3 P_OVER_2_232 > 2^24
    return x;
}
// the limbs of a canonical value packed into eight words
GPBC_INLINE void fr_words(uint32_t w[8], const Fr &x) {
    uint64_t acc = 0;
    int have = 0, wi = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        acc |= (uint64_t)(uint32_t)x.l.v[i] << have;
        have += LB;
        if (have >= 32 && wi < 8) { w[wi++] = (uint32_t)acc; acc >>= 32; have -= 32; }
    }
    if (wi < 8) w[wi] = (uint32_t)acc;
}
GPBC_INLINE void fr_store_canonical(uint8_t *p, const Fr &x) {
    uint32_t w[8];
    fr_words(w, x);
    uint32_t *q = reinterpret_cast<uint32_t *>(p);
#pragma unroll
    for (int i = 0; i < 8; i++) q[i] = w[i];
}
// plain value, reduced: one product by 2^261 mod r brings any loaded or summed value (|value| < 300 r) into (-eps r, (1 + eps) r)
GPBC_INLINE Fr fr_reduce(const Fr &a) { return fr_mul(a, fr_one()); }
GPBC_INLINE Fr fr_to_internal(const Fr &plain) { constexpr int32_t C[NL] = FR29_RSQ; return fr_mul(plain, fr_const(C)); }
// x == 0 (mod r), exactly, for a loaded value
GPBC_INLINE bool fr_is_zero(const Fr &a) { return fr_limbs_zero(fr_canonical<1, 2>(fr_reduce(a))); }
// OS2IP(64 bytes) mod r, canonical: fr.Element.SetBytes / hash.BytesToField on a 64-byte string, held in registers as the sixteen
// little-endian words of its bytes in order (a ChaCha20 block as it comes out).  Read big-endian the string is hi 2^256 + lo with
// hi = bytes 0..31 and lo = bytes 32..63: word k of a half is the byte-swapped word 7 - k of its bytes.  Both halves go through the
// scalar format's raw load (below 2^256 < 5.3 r each); hi 2^256 is ONE product with 2^517 mod r (mont(x, 2^517) = x 2^256, the
// constant of the fr.Element conversion), in (-eps r, (1 + eps) r); the sum with lo is below 6.3 r + eps r, and the canonical form
// subtracts r at most seven times.
GPBC_INLINE Fr fr_wide_reduce(const uint32_t (&w)[16]) {
    uint32_t hi[8], lo[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { hi[k] = __builtin_bswap32(w[7 - k]); lo[k] = __builtin_bswap32(w[15 - k]); }
    constexpr int32_t C[NL] = FR29_PLAIN_TO_MONT;
    const Fr top = fr_mul(fr_load_raw(reinterpret_cast<const uint8_t *>(hi)), fr_const(C));
    return fr_canonical<1, 7>(fr_add(top, fr_load_raw(reinterpret_cast<const uint8_t *>(lo))));
}

// ------------------------------------------------------------------------------------------------ inversion
// x -> 2^522 / x (the internal inverse of an internal x; 0 -> 0): fe_inv's safegcd with the modulus r.  The divsteps and the (f, g)
// update (inv30_divsteps, inv30_update_fg: fe29.hip.hpp, after libsecp256k1's modinv32, MIT) know no modulus and are used as they
// are; the (d, e) update and the final normalisation reduce modulo r here.  590 divsteps suffice for any odd modulus below 2^256.
GPBC_INLINE void fr_inv30_update_de(Inv30 &d, Inv30 &e, int32_t u, int32_t v, int32_t q, int32_t r) {
    constexpr int32_t M30 = 0x3fffffff;
    constexpr int32_t MOD[9] = INV30_R;
    const int32_t sd = d.v[8] >> 31, se = e.v[8] >> 31;
    int32_t md = (u & sd) + (v & se), me = (q & sd) + (r & se);
    int64_t cd = (int64_t)u * d.v[0] + (int64_t)v * e.v[0];
    int64_t ce = (int64_t)q * d.v[0] + (int64_t)r * e.v[0];
    md -= (int32_t)((INV30_RINV * (uint32_t)cd + (uint32_t)md) & (uint32_t)M30);
    me -= (int32_t)((INV30_RINV * (uint32_t)ce + (uint32_t)me) & (uint32_t)M30);
    cd += (int64_t)MOD[0] * md;
    ce += (int64_t)MOD[0] * me;
    cd >>= 30; ce >>= 30;
#pragma unroll
    for (int i = 1; i < 9; i++) {
        cd += (int64_t)u * d.v[i] + (int64_t)v * e.v[i] + (int64_t)MOD[i] * md;
        ce += (int64_t)q * d.v[i] + (int64_t)r * e.v[i] + (int64_t)MOD[i] * me;
        d.v[i - 1] = (int32_t)cd & M30; cd >>= 30;
        e.v[i - 1] = (int32_t)ce & M30; ce >>= 30;
    }
    d.v[8] = (int32_t)cd;
    e.v[8] = (int32_t)ce;
}
GPBC_INLINE void fr_inv30_normalize(Inv30 &r, int32_t sign) {
    constexpr int32_t M30 = 0x3fffffff;
    constexpr int32_t MOD[9] = INV30_R;
    int32_t add = r.v[8] >> 31;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] += MOD[i] & add;
    const int32_t neg = sign >> 31;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = (r.v[i] ^ neg) - neg;
#pragma unroll
    for (int i = 0; i < 8; i++) { r.v[i + 1] += r.v[i] >> 30; r.v[i] &= M30; }
    add = r.v[8] >> 31;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] += MOD[i] & add;
#pragma unroll
    for (int i = 0; i < 8; i++) { r.v[i + 1] += r.v[i] >> 30; r.v[i] &= M30; }
}
GPBC_INLINE Fr fr_inv(const Fr &x) {
    Fr c = fr_canonical<1, 2>(fr_mul(x, fr_one()));          // the stored integer A, canonical
    Inv30 g, f, d, e;
    {
        uint64_t acc = 0;
        int have = 0, wi = 0;
#pragma unroll
        for (int i = 0; i < NL; i++) {
            acc |= (uint64_t)(uint32_t)c.l.v[i] << have;
            have += LB;
            if (have >= 30 && wi < 9) { g.v[wi++] = (int32_t)(acc & 0x3fffffffu); acc >>= 30; have -= 30; }
        }
        if (wi < 9) g.v[wi] = (int32_t)acc;
    }
    constexpr int32_t MOD[9] = INV30_R;
#pragma unroll
    for (int i = 0; i < 9; i++) { f.v[i] = MOD[i]; d.v[i] = 0; e.v[i] = i == 0 ? 1 : 0; }
    int32_t zeta = -1;
    GPBC_B(bound_stats().mads += 20 * (6 * 9 + 4 * 9);)
    for (int it = 0; it < 20; it++) {
        int32_t u, v, q, r;
        zeta = inv30_divsteps(zeta, (uint32_t)f.v[0], (uint32_t)g.v[0], u, v, q, r);
        fr_inv30_update_de(d, e, u, v, q, r);
        inv30_update_fg(f, g, u, v, q, r);
    }
    fr_inv30_normalize(d, f.v[8]);
    Fr y;                                                    // d = A^-1 in [0, r), back in 29-bit limbs
    {
        uint64_t acc = 0;
        int have = 0, wi = 0;
#pragma unroll
        for (int i = 0; i < 9; i++) {
            acc |= (uint64_t)(uint32_t)d.v[i] << have;
            have += 30;
            while (have >= LB && wi < NL) { y.l.v[wi++] = (int32_t)(acc & (uint64_t)LMASK); acc >>= LB; have -= LB; }
        }
        if (wi < NL) y.l.v[wi] = (int32_t)acc;
    }
    GPBC_B(set_class_n(y.l, 1.0); y.lob = 0;)
    constexpr int32_t RC[NL] = FR29_RCUBE;
    return fr_mul(y, fr_const(RC));                          // A^-1 2^783 / 2^261 = 2^522 / A
}

// ------------------------------------------------------------------------------------------------ elementwise operations
// out = a OP b on the scalar format (the lane function of k_fr_op and of the host harness).  Every operation is products of the
// loaded limbs by constants: the sum / difference of two values below 2^256 is reduced by one product with 2^261 mod r, the
// product a b / 2^261 is multiplied back by 2^522, the Montgomery conversions of gnark's fr.Element (R = 2^256) are one product
// by 2^5 resp. 2^517.  b is ignored by the unary operations.
enum FrOp { FR_ADD = 0, FR_SUB = 1, FR_MUL = 2, FR_NEG = 3, FR_FROM_MONT = 4, FR_TO_MONT = 5, FR_OPS = 6 };
template <int OP> GPBC_INLINE void fr_op_lane(const uint8_t *pa, const uint8_t *pb, uint8_t *po) {
    const Fr a = fr_load_raw(pa);
    Fr r;
    if (OP == FR_ADD) r = fr_reduce(fr_add(a, fr_load_raw(pb)));
    else if (OP == FR_SUB) r = fr_reduce(fr_sub(a, fr_load_raw(pb)));
    else if (OP == FR_MUL) r = fr_to_internal(fr_mul(a, fr_load_raw(pb)));
    else if (OP == FR_NEG) r = fr_reduce(fr_neg(a));
    else if (OP == FR_FROM_MONT) { constexpr int32_t C[NL] = FR29_MONT_TO_PLAIN; r = fr_mul(a, fr_const(C)); }
    else { constexpr int32_t C[NL] = FR29_PLAIN_TO_MONT; r = fr_mul(a, fr_const(C)); }
    fr_store_canonical(po, fr_canonical<1, 2>(r));
}

// Inversion, gnark's Inverse (0 -> 0): a lane owns K elements (t, t + T, t + 2T, ..., T = ceil(n / K), as the group law does) and
// inverts the product of the K once (Montgomery's trick).  An element that is 0 modulo r puts 1 into the chain and gets 0, so it
// cannot spoil its neighbours.  The loaded values go into the chain unconverted: with stored x_j the chain holds
// P_j = x_0 ... x_j / 2^(261 j), fr_inv gives 2^522 / P_(K-1), walking back gives 2^522 / x_j, and one product by 2^-261 makes that
// the plain inverse — five products per element and 1 / K of an inversion.  Two passes keep the registers at the K prefix products
// (9 K VGPRs): pass 2 reads the element again; which elements are zero is carried over in one bit each.
// K = 8: 72 VGPRs of prefix products beside the ~60 of a product in flight fit three waves per SIMD (168 VGPRs) without scratch,
// and the inversion (~14 k instructions) is down to the cost of the element's own five products (~1.2 k) plus half as much again.
constexpr int FR_INV_K = 8;
template <int K> GPBC_INLINE void fr_inverse_lane(const uint8_t *a, uint8_t *out, size_t n, size_t t, size_t T) {
    static_assert(K >= 1 && K <= 32, "one zero bit per element");
    Fr pre[K];
    uint32_t zero = 0;
#pragma unroll
    for (int j = 0; j < K; j++) {
        const size_t i = t + (size_t)j * T;
        Fr x = fr_one();                                    // 2^261: the chain's 1 (P_j = P_(j-1) exactly)
        bool z = true;
        if (i < n) {
            const Fr v = fr_load_raw(a + 32 * i);
            z = fr_is_zero(v);
            if (!z) x = v;
        }
        zero |= (uint32_t)z << j;
        pre[j] = j ? fr_mul(pre[j > 0 ? j - 1 : 0], x) : x;
    }
    Fr inv = fr_inv(pre[K - 1]);
    constexpr int32_t C[NL] = FR29_INV_RP;
#pragma unroll
    for (int j = K - 1; j >= 0; j--) {
        const size_t i = t + (size_t)j * T;
        if (i >= n) continue;                               // padding: the chain carried a 1, inv stays as it is
        if ((zero >> j) & 1u) { fr_store_canonical(out + 32 * i, fr_zero()); continue; }
        const Fr x = fr_load_raw(a + 32 * i);
        const Fr xinv = j ? fr_mul(inv, pre[j > 0 ? j - 1 : 0]) : inv;      // 2^522 / x
        if (j) inv = fr_mul(inv, x);
        fr_store_canonical(out + 32 * i, fr_canonical<1, 2>(fr_mul(xinv, fr_const(C))));
    }
}

// ------------------------------------------------------------------------------------------------ polynomials
// Coefficients are kept plain.  The steps below are the whole arithmetic of k_fr_poly_from_roots / k_fr_poly_quotients; the kernels
// (csrc/gpbc_fr.hip) and the host harness (tools/bounds_check.cpp) differ only in where the values wait between steps.
constexpr int FR_POLY_MAX_B = 1024;
// a root, loaded: -root in internal form (computePolynomialCoeffs multiplies by the negated identity)
GPBC_INLINE Fr fr_poly_neg_root(const uint8_t *p) { return fr_neg(fr_to_internal(fr_load_raw(p))); }
// one step of prod (X - root): new c_i = c_(i-1) - root c_i as ONE reduction, (c_(i-1) 2^261 + (-root 2^261) c_i) / 2^261, so the
// value never drifts however many steps follow (in and out: product class, |value| < 1.1 r)
GPBC_INLINE Fr fr_poly_root_step(const Fr &c_below, const Fr &c_i, const Fr &neg_root) { return fr_mul2(c_below, fr_one(), neg_root, c_i); }
GPBC_INLINE void fr_poly_store(uint8_t *p, const Fr &c) { fr_store_canonical(p, fr_canonical<1, 2>(c)); }
// f's coefficient as the division reads it: canonical (so that a step's sum stays below 3 r)
GPBC_INLINE Fr fr_poly_coeff_in(const uint8_t *p) { return fr_canonical<1, 2>(fr_reduce(fr_load_raw(p))); }
GPBC_INLINE Fr fr_poly_point(const uint8_t *p) { return fr_to_internal(fr_load_raw(p)); }
// one step of the synthetic division: carry <- c_i + carry point, canonical — it is the quotient's coefficient i - 1 as it is
// written, and after the last step (i = 0) the remainder f(point)
GPBC_INLINE Fr fr_poly_horner_step(const Fr &carry, const Fr &c_i, const Fr &point) { return fr_canonical<1, 3>(fr_add(c_i, fr_mul(carry, point))); }

// ------------------------------------------------------------------------------------------------ Lagrange basis
// out[t] = prod over the set elements s != node_t (by value modulo r) of (x - s) / (node_t - s): utils.ComputeLagrangeBasis of the
// reference as fibe/sw05_fibe_common.go:316 and fibe/sw05_fibe_large_universe.go:277,318 call it, once per element of a set that
// differs from item to item.  Set elements, nodes and x are made canonical ONCE (fr_lagrange_in, when the set is staged and when a
// lane loads its node), so "s equals the node" is a limb comparison and a factor is the carry-free difference of two canonical
// values.  A skipped factor multiplies both products by the chain's 1 (2^261), which keeps every lane of a wave on one path.
// Numerator and denominator start at 2^261 and take the same number c of plain factors, so both are (true value) x 2^(261 (1 - c))
// and the power cancels in the quotient: no factor is ever converted.
// A lane owns G outputs of ONE row (nodes gi, gi + gpr, ..., gpr = ceil(m / G): neighbouring lanes read and write neighbouring
// scalars) and inverts the product of their G denominators once.  With D_g, N_g the products of output g:
//   P_g = P_(g-1) D_g / 2^261,  W_g = N_g P_(g-1) / 2^261  (P_0 = D_0, W_0 = N_0),  I_(G-1) = 2^261 / P_(G-1) (fr_inv and one product),
//   out_g = W_g I_g / 2^261 = N_g / D_g,  I_(g-1) = I_g D_g / 2^261 = 2^261 / P_(g-1)
// — four products per output beside its 2 B and 1 / G of an inversion; W and D wait in registers (18 G VGPRs).  An output past
// the row's end carries D = 2^261 and leaves the chain as it is.  No denominator is 0 (every factor equal to the node is skipped),
// so there is nothing to flag.  G = 4: 72 VGPRs of W and D beside node, x, the two running products and a product in flight; the
// inversion (~14 k instructions) is then 3.5 k per output against the 2 B + 4 products (~8 k at B = 16).
constexpr int FR_LAGRANGE_G = 4;
GPBC_INLINE Fr fr_lagrange_in(const uint8_t *p) { return fr_canonical<1, 2>(fr_reduce(fr_load_raw(p))); }
GPBC_INLINE bool fr_limbs_equal(const Fr &a, const Fr &b) {       // of two canonical values
    int32_t o = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) o |= a.l.v[i] ^ b.l.v[i];
    return o == 0;
}
// set_at(u): the canonical set element u of the lane's row (LDS on the device, a vector in the host harness); nodes: the row's m
// nodes in the scalar format, or null = the set's own elements (m == B); out: the row's m outputs.
template <int G, class SetAt>
GPBC_INLINE void fr_lagrange_lane(const SetAt &set_at, uint32_t B, const uint8_t *nodes, const Fr &x, uint32_t m, uint32_t gi, uint32_t gpr, uint8_t *out) {
    Fr W[G], D[G], P = fr_one();
#pragma unroll
    for (int g = 0; g < G; g++) {
        const uint32_t t = gi + (uint32_t)g * gpr;
        Fr n = fr_one(), d = fr_one();
        if (t < m) {
            const Fr node = nodes ? fr_lagrange_in(nodes + 32 * (size_t)t) : set_at(t);
            for (uint32_t u = 0; u < B; u++) {
                const Fr s = set_at(u);
                const bool skip = fr_limbs_equal(s, node);
                n = fr_mul(n, skip ? fr_one() : fr_sub(x, s));
                d = fr_mul(d, skip ? fr_one() : fr_sub(node, s));
            }
        }
        D[g] = d;
        W[g] = g ? fr_mul(n, P) : n;
        P = g ? fr_mul(P, d) : d;
    }
    Fr inv = fr_mul(fr_inv(P), fr_plain_one());                // 2^522 / P / 2^261
#pragma unroll
    for (int g = G - 1; g >= 0; g--) {
        const uint32_t t = gi + (uint32_t)g * gpr;
        if (t < m) fr_store_canonical(out + 32 * (size_t)t, fr_canonical<1, 2>(fr_mul(W[g], inv)));
        if (g) inv = fr_mul(inv, D[g]);
    }
}

// The launch of k_fr_lagrange_basis (csrc/gpbc_fr.hip), in functions the host harness runs as well: one wave of FR_LAG_WAVE lanes per
// workgroup, gpr = ceil(m / G) lanes per row, rpb rows per workgroup (or bpr workgroups per row when gpr > 64), the sets of a
// workgroup's rows staged at word offset (local row) x pitch + u x NL of an LDS block of cap x NL + FR_LAG_WAVE words, cap = 256 or 1024
// set elements.  The pitch is odd, so the rows of a wave start in different banks.
constexpr int FR_LAG_WAVE = 64, FR_LAG_SMALL = 256, FR_LAG_LARGE = FR_POLY_MAX_B;
struct LagrangeGeom { uint32_t B, m, gpr, rpb, bpr, large; };
struct LagrangeLane { size_t row; uint32_t lr, gi; bool active; };
// rows per workgroup lowered until their sets fit; only B > 16 with m < 64 and a set per row leaves lanes idle
inline LagrangeGeom fr_lagrange_geometry(size_t B, size_t m, bool shared_set) {
    LagrangeGeom g;
    g.B = (uint32_t)B; g.m = (uint32_t)m;
    g.gpr = (uint32_t)((m + FR_LAGRANGE_G - 1) / FR_LAGRANGE_G);
    g.bpr = (g.gpr + FR_LAG_WAVE - 1) / FR_LAG_WAVE;
    g.rpb = g.bpr > 1 ? 1 : FR_LAG_WAVE / g.gpr;
    const size_t need = shared_set ? B : g.rpb * B;
    g.large = need > (size_t)FR_LAG_SMALL;
    if (need > (size_t)FR_LAG_LARGE) g.rpb = (uint32_t)((size_t)FR_LAG_LARGE / B);        // >= 1: B <= 1024
    return g;
}
GPBC_INLINE uint32_t fr_lagrange_pitch(const LagrangeGeom &g) { return (g.B * NL) | 1u; }
GPBC_INLINE size_t fr_lagrange_row0(const LagrangeGeom &g, uint32_t block) { return (size_t)(block / g.bpr) * g.rpb; }
GPBC_INLINE uint32_t fr_lagrange_rows(const LagrangeGeom &g, uint32_t block, size_t k) {
    const size_t left = k - fr_lagrange_row0(g, block);
    return left < g.rpb ? (uint32_t)left : g.rpb;
}
// a lane's share of the staging: put(word offset, canonical element); set_step = 0 stages the one shared set
template <class Put> GPBC_INLINE void fr_lagrange_stage(const LagrangeGeom &g, uint32_t block, uint32_t lane, size_t k, const uint8_t *set, size_t set_step, const Put &put) {
    const size_t row0 = fr_lagrange_row0(g, block);
    const uint32_t staged = set_step ? fr_lagrange_rows(g, block, k) : 1u, pitch = fr_lagrange_pitch(g);
    for (uint32_t idx = lane; idx < staged * g.B; idx += FR_LAG_WAVE) {
        const uint32_t lr = idx / g.B, u = idx % g.B;
        put(lr * pitch + u * NL, fr_lagrange_in(set + (row0 + lr) * set_step + 32 * (size_t)u));
    }
}
GPBC_INLINE LagrangeLane fr_lagrange_map(const LagrangeGeom &g, uint32_t block, uint32_t lane, size_t k) {
    LagrangeLane l;
    l.lr = lane / g.gpr;
    l.gi = (block % g.bpr) * FR_LAG_WAVE + lane % g.gpr;
    l.row = fr_lagrange_row0(g, block) + l.lr;
    l.active = l.lr < fr_lagrange_rows(g, block, k) && l.gi < g.gpr;
    return l;
}
GPBC_INLINE size_t fr_lagrange_grid(const LagrangeGeom &g, size_t k) { return (k + g.rpb - 1) / g.rpb * g.bpr; }

// ------------------------------------------------------------------------------------------------ LSSS reconstruction weights
// w with sum_x w_x M_x = (1, 0, ..., 0) over the rows x of an LSSS matrix that a key holds, one system per ciphertext:
// FindLinearCombinationWeight of the reference (access/lsss/lewko_waters_lsss_matrix.go:167-429) as cpabe/waters11 Decrypt calls it
// (waters11_cpabe.go:254).  The result is DEFINED, so that it is unique: the held rows in ascending order, a row is used iff its vector
// is independent of the used rows before it (the greedy first basis), w is the one combination of the used rows that gives the target
// and 0 everywhere else; ok = 0 and w = 0 when the target is not in their span.  That is lw11.reconstruction_weights spread over all
// rows; it does not depend on which equation an elimination takes as pivot.
//
// Gauss-Jordan on the transposed augmented matrix: `cols` equations, one unknown per row of M and the right-hand side e_0 as
// column `rows`.  A group of gw = max(rows + 1, cols) lanes owns one system, lane li of the group owns column li (rows = 64: the
// right-hand side is a second column of lane 0, gw = 64); a wave holds spw = 64 / gw systems.  The columns live in LDS (the pivot
// equation is indexed at run time): column j of local system ls at word ls x sys_words + j x pitch, equation i at + i x NL, pitch odd.
// A row that is not held is staged as zeros and so never gets a pivot.
//   step c (one per unknown, in ascending order): lane li < cols tests element (equation li, column c) for == 0 mod r exactly
//   (canonical form: r itself and a lazily reduced multiple of r count as zero); the group's slice of the wave's ballot is the set
//   of non-zero equations; the pivot is the lowest one not yet used (none: the row is dependent, weight 0).  Every OTHER non-zero
//   equation i is eliminated fraction-free, a[i][j] <- (p a[i][j] - f_i a[pivot][j]) / 2^261, one fr_mul2 per element, no
//   inversion; an equation with f_i == 0 is left as it is.  Scaling an equation scales its right-hand side alike, so neither the
//   factor p nor the 2^-261 of the product changes the solution.  Nobody writes column c during the step (it holds the factors
//   every lane reads); its owner zeroes it after a barrier, all but the pivot (fr_lsss_clear).
//   finish: ok iff the right-hand side is 0 in every unused equation; a lane with a pivot returns rhs[pivot] / a[pivot][own column],
//   one lane-parallel fr_inv per wave.
// The lanes of a group branch alike; groups of one wave differ only in which equations their loops visit (no cross-lane operation
// inside).  The ballots are taken with every lane present.
constexpr int FR_LSSS_MAX = 64, FR_LSSS_WAVE = 64, FR_LSSS_NONE = 0xff;
// LDS instances of the kernel (words of the block): 29 KB = three 16 x 16 systems, five workgroups per CU; 80 KB = one system up to
// 46 x 46, two per CU; 146.5 KB = one 64 x 64 system, alone on its CU
constexpr int FR_LSSS_WORDS_0 = 7424, FR_LSSS_WORDS_1 = 20480, FR_LSSS_WORDS_2 = (FR_LSSS_MAX + 1) * ((FR_LSSS_MAX * NL) | 1);
GPBC_INLINE constexpr int fr_lsss_words(uint32_t level) { return level == 0 ? FR_LSSS_WORDS_0 : level == 1 ? FR_LSSS_WORDS_1 : FR_LSSS_WORDS_2; }
struct LsssGeom { uint32_t rows, cols, gw, spw, pitch, sys_words, level; };
struct LsssLane { size_t sys; uint32_t base, li, shift; bool active; };
struct LsssState { uint64_t unused; uint32_t pivot; };
inline LsssGeom fr_lsss_geometry(size_t rows, size_t cols) {
    LsssGeom g;
    g.rows = (uint32_t)rows; g.cols = (uint32_t)cols;
    g.gw = (uint32_t)(rows + 1 > cols ? rows + 1 : cols);
    if (g.gw > FR_LSSS_WAVE) g.gw = FR_LSSS_WAVE;
    g.pitch = (g.cols * NL) | 1u;
    g.sys_words = (g.rows + 1) * g.pitch;
    g.spw = FR_LSSS_WAVE / g.gw;
    g.level = g.sys_words <= (uint32_t)FR_LSSS_WORDS_0 ? 0 : g.sys_words <= (uint32_t)FR_LSSS_WORDS_1 ? 1 : 2;
    if (g.spw * g.sys_words > (uint32_t)fr_lsss_words(g.level)) g.spw = (uint32_t)fr_lsss_words(g.level) / g.sys_words;      // >= 1
    return g;
}
GPBC_INLINE size_t fr_lsss_grid(const LsssGeom &g, size_t k) { return (k + g.spw - 1) / g.spw; }
GPBC_INLINE uint32_t fr_lsss_systems(const LsssGeom &g, uint32_t block, size_t k) {
    const size_t left = k - (size_t)block * g.spw;
    return left < g.spw ? (uint32_t)left : g.spw;
}
// a lane's share of the staging: put(word offset, value).  mat_step = 0: one matrix for every system.
template <class Put> GPBC_INLINE void fr_lsss_stage(const LsssGeom &g, uint32_t block, uint32_t lane, size_t k, const uint8_t *matrix, size_t mat_step, const uint8_t *held, const Put &put) {
    const size_t sys0 = (size_t)block * g.spw;
    const uint32_t per = (g.rows + 1) * g.cols, total = fr_lsss_systems(g, block, k) * per;
    for (uint32_t idx = lane; idx < total; idx += FR_LSSS_WAVE) {
        const uint32_t ls = idx / per, j = (idx % per) / g.cols, i = idx % g.cols;
        Fr v = fr_zero();
        if (j == g.rows) { if (i == 0) v = fr_plain_one(); }
        else if (held[(sys0 + ls) * g.rows + j]) v = fr_lagrange_in(matrix + (sys0 + ls) * mat_step + 32 * ((size_t)j * g.cols + i));
        put(ls * g.sys_words + j * g.pitch + i * NL, v);
    }
}
GPBC_INLINE LsssLane fr_lsss_map(const LsssGeom &g, uint32_t block, uint32_t lane, size_t k) {
    LsssLane l;
    const uint32_t ls = lane / g.gw;
    l.li = lane % g.gw;
    l.shift = ls * g.gw;
    l.base = ls * g.sys_words;
    l.sys = (size_t)block * g.spw + ls;
    l.active = ls < fr_lsss_systems(g, block, k);
    if (!l.active) { l.base = 0; l.shift = 0; }
    return l;
}
GPBC_INLINE LsssState fr_lsss_begin(const LsssGeom &g) {
    LsssState s;
    s.unused = g.cols == 64 ? ~(uint64_t)0 : (((uint64_t)1 << g.cols) - 1);
    s.pivot = FR_LSSS_NONE;
    return s;
}
// the lane's ballot bit: element (equation li, column col) of its system is not 0 modulo r
template <class Get> GPBC_INLINE bool fr_lsss_nonzero(const LsssGeom &g, const LsssLane &l, uint32_t col, const Get &get) {
    if (!l.active || l.li >= g.cols) return false;
    return !fr_limbs_zero(fr_canonical<1, 2>(get(l.base + col * g.pitch + l.li * NL)));
}
GPBC_INLINE uint32_t fr_lsss_ctz(uint64_t v) { return (uint32_t)__builtin_ctzll(v); }       // v != 0
template <class Get, class Put> GPBC_INLINE void fr_lsss_step(const LsssGeom &g, const LsssLane &l, uint32_t c, uint64_t ballot, LsssState &s, const Get &get, const Put &put) {
    const uint64_t all = g.cols == 64 ? ~(uint64_t)0 : (((uint64_t)1 << g.cols) - 1);
    const uint64_t nz = (ballot >> l.shift) & all, cand = nz & s.unused;
    if (!l.active || !cand) return;
    const uint32_t p = fr_lsss_ctz(cand);
    s.unused &= ~((uint64_t)1 << p);
    if (l.li == c) s.pivot = p;
    const uint32_t fcol = l.base + c * g.pitch;
    const Fr pv = get(fcol + p * NL);
    for (uint64_t el = nz & ~((uint64_t)1 << p); el; el &= el - 1) {
        const uint32_t i = fr_lsss_ctz(el);
        const Fr nf = fr_neg(get(fcol + i * NL));
        for (uint32_t j = l.li; j <= g.rows; j += FR_LSSS_WAVE) {
            if (j == c) continue;
            const uint32_t cj = l.base + j * g.pitch;
            put(cj + i * NL, fr_mul2_inline(pv, get(cj + i * NL), nf, get(cj + p * NL)));
        }
    }
}
// after the step, once every lane of the group has read its factors: the owner of column c leaves only the pivot in it
template <class Put> GPBC_INLINE void fr_lsss_clear(const LsssGeom &g, const LsssLane &l, uint32_t c, const LsssState &s, const Put &put) {
    if (!l.active || l.li != c || s.pivot == FR_LSSS_NONE) return;
    for (uint32_t i = 0; i < g.cols; i++)
        if (i != s.pivot) put(l.base + c * g.pitch + i * NL, fr_zero());
}
// ballot: fr_lsss_nonzero of the right-hand side (column `rows`)
template <class Get> GPBC_INLINE void fr_lsss_finish(const LsssGeom &g, const LsssLane &l, uint64_t ballot, const LsssState &s, const Get &get, uint8_t *w_out, uint8_t *ok_out) {
    const bool ok = l.active && !((ballot >> l.shift) & s.unused), mine = ok && l.li < g.rows && s.pivot != FR_LSSS_NONE;
    Fr den = fr_one(), num = fr_zero();
    if (mine) {
        den = get(l.base + l.li * g.pitch + s.pivot * NL);
        num = get(l.base + g.rows * g.pitch + s.pivot * NL);
    }
    const Fr w = fr_mul(num, fr_mul(fr_inv(den), fr_plain_one()));             // num x (2^522 / den / 2^261) / 2^261
    if (!l.active) return;
    if (l.li < g.rows) fr_store_canonical(w_out + 32 * (l.sys * g.rows + l.li), fr_canonical<1, 2>(w));
    if (l.li == 0) ok_out[l.sys] = ok ? 1 : 0;
}

}  // namespace gpbc
#endif
