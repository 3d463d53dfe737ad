// Elementwise group law on affine points, G1 (Fp) and G2 (the twist, Fp2): out[i] = a[i] + b[j], a[i] - b[j], 2 a[i]
// (j = i, or j = 0 for a broadcast b).  Replaces gnark-crypto's G1Affine / G2Affine Add, Sub and Double as the reference
// calls them between device-resident steps of its schemes (cpabe/bsw07/bsw07_cpabe.go:104,119, dabe/lw11_dabe.go:100,157,
// cpabe/waters11/waters11_cpabe.go:226, signature/zss04_signature/zss04_signature.go:327, ...).
//
// Affine formulas, lambda = (y_b - y_a) / (x_b - x_a) or 3 x_a^2 / (2 y_a), x3 = lambda^2 - x_a - x_b, y3 = lambda (x_a - x3) - y_a:
// about four products per element, but one division.  An inversion (safegcd, ~45 Fp products) per element would be 90 % of
// the work, so a lane owns K elements (t, t+T, t+2T, ... with T = ceil(n / K): neighbouring lanes read neighbouring rows)
// and inverts the product of their K denominators ONCE (Montgomery's trick: prefix products, one inversion, walk back).
// An element whose result needs no division (an input at infinity, P + (-P), the padding past n) puts 1 into the chain, so
// it cannot spoil its neighbours.
//
// No conversions: coordinates are taken into the internal form as they are and left there.  gnark's bytes hold x 2^256 mod p
// and the internal Montgomery radix is 2^261, so the limbs of those bytes, read unconverted, ARE the internal form of c x with
// c = 2^-5 — and the internal form of c x3 is, written back unconverted, gnark's bytes of x3.  The formulas run on the c-scaled
// coordinates: c x_b - c x_a = c (x_b - x_a); the lane's one inverse is multiplied by c once, so that num / den comes out as
// c lambda; lambda itself is 32 (c lambda) (32 c = 1: a few shifts); c x3 = (c lambda) lambda - c x_a - c x_b and
// c y3 = lambda (c x_a - c x3) - c y_a.  That saves the six conversion products (two per point read, one per coordinate
// written) an element would otherwise cost beside its five.
//
// Two passes over the lane's K elements keep the register footprint at the K prefix products: pass 1 reads what decides
// the element's case (the raw infinity test, the x coordinates; the y coordinates only when the x coordinates agree) and
// multiplies its denominator into the chain; pass 2, walking back, reads the element again and finishes it.  The case is
// carried from pass 1 to pass 2 in 3 bits per element, so the exact zero tests run once.
//
// Semantics are gnark's: the all-zero encoding is infinity (decided on the raw bytes, as g1_load_aff does); P + inf = P,
// P + P doubles, P + (-P) = inf, written as all zero; outputs are canonical.  The affine result is unique, so it is
// bit-identical to gnark.  out may be a (or b with one b per element): every element reads its own rows before it writes
// its own output row, and no other element touches them.
#ifndef GPBC_GROUP29_HIP_HPP
#define GPBC_GROUP29_HIP_HPP
#include "curve29.hip.hpp"

namespace gpbc {

enum GroupOp { GROUP_ADD = 0, GROUP_SUB = 1, GROUP_DBL = 2 };
// the case of one element, decided in pass 1
enum : uint32_t { GM_LINE = 0, GM_TANGENT = 1, GM_INF = 2, GM_COPY_A = 3, GM_COPY_B = 4, GM_NONE = 5 };
constexpr int GM_BITS = 3;
// Elements per lane that share one field inversion (the kernels of gpbc_group.hip and the host harness tools/bounds_check.cpp).
// The lane holds its K prefix products (K x 9 / 18 VGPRs) across the inversion; the rest of its state is re-read in pass 2.
// A lane's work is one long dependent chain, so what decides the speed is how many waves each SIMD holds at once: K is chosen
// so that 2^20 elements make ONE round of resident waves (G1: 3 per SIMD, 2^20 / (64 x 6) = 2731 waves on 1024 SIMDs; G2: 2,
// 2048 waves).  Resource report and timings: DESIGN.md §10.
constexpr int GROUP_K_G1 = 6, GROUP_K_G2 = 8;
template <class F> constexpr int group_k() { return sizeof(F) == sizeof(Fe) ? GROUP_K_G1 : GROUP_K_G2; }

// unconverted load / store of one coordinate: the internal form of c x (see above); the store makes it canonical
GPBC_INLINE Fe fe_load_raw(const uint8_t *p) {
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = q[i];
    Fe x;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        int bit = LB * i, wi = bit >> 5, sh = bit & 31;
        uint64_t two = (uint64_t)w[wi] | ((wi + 1 < 8) ? ((uint64_t)w[wi + 1] << 32) : 0);
        x.v[i] = (int32_t)((two >> sh) & (uint64_t)LMASK);
    }
    GPBC_B(set_class_n(x, 1.0);)                          // canonical input: value < p
    return x;
}
// [0, p) from |value| < p (weakly normalised limbs): add p, carry, subtract p once if that leaves no borrow — fe_canonical
// without its eight rounds for the (-4p, 4p) range
GPBC_INLINE Fe fe_canonical_small(const Fe &a) {
    int32_t t[NL];
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < NL - 1; i++) { int64_t s = (int64_t)a.v[i] + (int64_t)f29_p(i) + c; t[i] = (int32_t)(s & LMASK); c = s >> LB; }
    t[NL - 1] = (int32_t)((int64_t)a.v[NL - 1] + (int64_t)f29_p(NL - 1) + c);
    int32_t d[NL], b = 0;
#pragma unroll
    for (int i = 0; i < NL - 1; i++) { int32_t s = t[i] - f29_p(i) + b; d[i] = s & LMASK; b = s >> LB; }
    d[NL - 1] = t[NL - 1] - f29_p(NL - 1) + b;
    const bool ge = d[NL - 1] >= 0;
    Fe r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.v[i] = ge ? d[i] : t[i];
#ifdef GPBC_BOUNDS
    if (a.vb >= 1.0) bounds_fail("fe_canonical_small input value", a.vb, 1.0);
    set_class_n(r, 1.0);
#endif
    return r;
}
GPBC_INLINE void fe_store_raw(uint8_t *p, const Fe &a) {
    Fe x = fe_canonical_small(fe_reduce_arith_norm(a));    // (|value| < 256 p in; 0.51 p after the reduction)
    uint32_t w[8];
    uint64_t acc = 0;
    int have = 0, wi = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        acc |= (uint64_t)(uint32_t)x.v[i] << have;
        have += LB;
        if (have >= 32 && wi < 8) { w[wi++] = (uint32_t)acc; acc >>= 32; have -= 32; }
    }
    if (wi < 8) w[wi] = (uint32_t)acc;
    uint32_t *q = reinterpret_cast<uint32_t *>(p);
#pragma unroll
    for (int i = 0; i < 8; i++) q[i] = w[i];
}
// 32 a: normalised doublings and one shift by three (limbs stay inside int32 for an N-class input)
GPBC_INLINE Fe fe_mul32_norm(const Fe &a) { return fe_mul8_norm(fe_norm(fe_dbl(fe_norm(fe_dbl(a))))); }
GPBC_INLINE F2 f2_mul32_norm(const F2 &a) { return F2{fe_mul32_norm(a.a0), fe_mul32_norm(a.a1)}; }
GPBC_INLINE Fe g_mul32(const Fe &a) { return fe_mul32_norm(a); }
GPBC_INLINE F2 g_mul32(const F2 &a) { return f2_mul32_norm(a); }
// times c = 2^-5: the internal form of c is 2^256 mod p
GPBC_INLINE Fe g_mul_c(const Fe &a) { constexpr int32_t C[NL] = F29_FROM_INTERNAL; return fe_mul(a, fe_const(C)); }
GPBC_INLINE F2 g_mul_c(const F2 &a) { constexpr int32_t C[NL] = F29_FROM_INTERNAL; return f2_mul_fe(a, fe_const(C)); }

template <class F> struct GroupPt;
template <> struct GroupPt<Fe> {
    static constexpr size_t BYTES = 64, COORD = 32;
    static GPBC_INLINE Fe ld(const uint8_t *p) { return fe_load_raw(p); }
    static GPBC_INLINE void st(uint8_t *p, const Fe &v) { fe_store_raw(p, v); }
};
template <> struct GroupPt<F2> {
    static constexpr size_t BYTES = 128, COORD = 64;
    static GPBC_INLINE F2 ld(const uint8_t *p) { return F2{fe_load_raw(p), fe_load_raw(p + 32)}; }
    static GPBC_INLINE void st(uint8_t *p, const F2 &v) { fe_store_raw(p, v.a0); fe_store_raw(p + 32, v.a1); }
};

// dst <- src, `words` 32-bit words (dst may equal src)
GPBC_INLINE void group_copy_words(uint8_t *dst, const uint8_t *src, int words) {
    const uint32_t *s = reinterpret_cast<const uint32_t *>(src);
    uint32_t *d = reinterpret_cast<uint32_t *>(dst);
    for (int i = 0; i < words; i++) d[i] = s[i];
}
GPBC_INLINE void group_zero_words(uint8_t *dst, int words) {
    uint32_t *d = reinterpret_cast<uint32_t *>(dst);
    for (int i = 0; i < words; i++) d[i] = 0;
}

// Pass 1 for one element: its case and its denominator (x_b - x_a, or 2 y_a for a doubling; 1 where there is none).
// N-class denominator.
template <class F, int OP> GPBC_INLINE uint32_t group_classify(F &den, const uint8_t *pa, const uint8_t *pb) {
    using IO = GroupPt<F>;
    constexpr int W = (int)(IO::BYTES / 4);
    g_set_one(den);
    const bool ainf = bytes_all_zero(pa, W);
    if (OP == GROUP_DBL) {
        if (ainf) return GM_INF;
        F d = g_norm(g_dbl(IO::ld(pa + IO::COORD)));
        if (g_is_zero(d)) return GM_INF;                 // y = 0: order two (no such point in either group; kept total)
        den = d;
        return GM_TANGENT;
    }
    const bool binf = bytes_all_zero(pb, W);
    if (ainf) return binf ? GM_INF : GM_COPY_B;
    if (binf) return GM_COPY_A;
    F dx = g_norm(g_sub(IO::ld(pb), IO::ld(pa)));
    if (!g_is_zero(dx)) { den = dx; return GM_LINE; }
    // same x: b' = a doubles, b' = -a gives infinity (b' = b, or -b for SUB)
    F ya = IO::ld(pa + IO::COORD), yb = IO::ld(pb + IO::COORD);
    F s = OP == GROUP_SUB ? g_norm(g_add(yb, ya)) : g_norm(g_sub(yb, ya));
    if (!g_is_zero(s)) return GM_INF;
    F d = g_norm(g_dbl(ya));
    if (g_is_zero(d)) return GM_INF;
    den = d;
    return GM_TANGENT;
}

// One lane: elements i = t + j T (j < K, i < n) of out = a OP b, b read at i * b_step (b_step = 0: one b for all).
template <class F, int K, int OP> GPBC_INLINE void group_op_lane(const uint8_t *a, const uint8_t *b, size_t b_step, uint8_t *out, size_t n, size_t t, size_t T) {
    using IO = GroupPt<F>;
    constexpr int W = (int)(IO::BYTES / 4), WC = (int)(IO::COORD / 4);
    static_assert(K >= 1 && K * GM_BITS <= 64, "the cases of a lane's elements are packed into one 64-bit word");
    F pre[K];                                            // pre[j] = den_0 ... den_j
    uint64_t modes = 0;
#pragma unroll
    for (int j = 0; j < K; j++) {
        const size_t i = t + (size_t)j * T;
        F den;
        uint32_t m = GM_NONE;
        g_set_one(den);
        if (i < n) m = group_classify<F, OP>(den, a + i * IO::BYTES, OP == GROUP_DBL ? a + i * IO::BYTES : b + i * b_step);
        modes |= (uint64_t)m << (GM_BITS * j);
        pre[j] = j ? g_mul(pre[j - 1], den) : den;
    }
    F inv = g_mul_c(g_inv(pre[K - 1]));                  // c / (den_0 ... den_{K-1})
#pragma unroll
    for (int j = K - 1; j >= 0; j--) {
        const size_t i = t + (size_t)j * T;
        const uint32_t m = (uint32_t)(modes >> (GM_BITS * j)) & 7u;
        const uint8_t *pa = a + i * IO::BYTES, *pb = OP == GROUP_DBL ? pa : b + i * b_step;
        uint8_t *po = out + i * IO::BYTES;
        if (m == GM_LINE || m == GM_TANGENT) {
            // all coordinates c-scaled; num is c times the numerator of lambda
            F xa = IO::ld(pa), ya = IO::ld(pa + IO::COORD), xb, num, den;
            if (m == GM_LINE) {
                F yb = IO::ld(pb + IO::COORD);
                xb = IO::ld(pb);
                den = g_norm(g_sub(xb, xa));
                num = OP == GROUP_SUB ? g_norm(g_neg(g_add(yb, ya))) : g_norm(g_sub(yb, ya));
            } else {
                F xx = g_sqr(xa);                                   // c^2 x^2
                xb = xa;
                den = g_norm(g_dbl(ya));
                num = g_mul32(g_norm(g_add(g_dbl(xx), xx)));        // 32 * 3 c^2 x^2 = c 3 x^2
            }
            const F dinv = j ? g_mul(inv, pre[j > 0 ? j - 1 : 0]) : inv;     // c / den
            if (j) inv = g_mul(inv, den);
            const F lam_c = g_mul(num, dinv);                      // c lambda
            const F lam = g_mul32(lam_c);                          // lambda
            const F x3 = g_norm(g_sub(g_sub(g_mul(lam_c, lam), xa), xb));
            const F y3 = g_sub(g_mul(lam, g_sub(xa, x3)), ya);     // differences of normalised values: no normalisation needed
            IO::st(po, x3);
            IO::st(po + IO::COORD, y3);
            continue;
        }
        // no division: the chain carried a 1 for this element, inv stays as it is
        if (m == GM_INF) group_zero_words(po, W);
        else if (m == GM_COPY_A) group_copy_words(po, pa, W);
        else if (m == GM_COPY_B && OP != GROUP_SUB) group_copy_words(po, pb, W);
        else if (m == GM_COPY_B) {                              // -b: (x, -y), canonical
            const F yb = IO::ld(pb + IO::COORD);
            group_copy_words(po, pb, WC);
            IO::st(po + IO::COORD, g_neg(yb));
        }
    }
}

}  // namespace gpbc
#endif
