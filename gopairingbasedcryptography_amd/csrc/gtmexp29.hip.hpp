// Segmented multi-exponentiation in GT on a lane pair: out = prod_i x_i^{k_i} over a run of factors, with GT.Exp's semantics per
// factor (f12p_exp256: 256-bit plain exponents, any Fp12 base, fixed 4-bit windows left to right) and ONE squaring chain for
// GT_MEXP_GROUP factors (Straus interleaving): the factors are taken four at a time, each with its 16-row window table, and a
// window costs 4 squarings + 4 table products for the four of them — 63 + 77.25 x 2.34 = 244 squaring-equivalents per factor
// where f12p_exp256 spends 252 + 77 x 2.34 = 432.  The tables of ONE group are the whole workspace of a lane (GT_MEXP_TAB_DWORDS
// int32, 16 KB), whatever the length of the run: the next group overwrites them.
// The work is cut by csrc/segred29.hip.hpp with GT_MEXP_SHAPE (one lane pair per piece): the kernels (csrc/gpbc_gtmexp.hip) and the host
// interval harness (tools/bounds_check.cpp, hc_gt_multi_exp_pair) run one plan.
#ifndef GPBC_GTMEXP29_HIP_HPP
#define GPBC_GTMEXP29_HIP_HPP
#include "pairing29_pair.hip.hpp"
#include "segred29.hip.hpp"

namespace gpbc {

constexpr int GT_MEXP_GROUP = 4;                                             // factors that share a squaring chain
constexpr int GT_MEXP_TAB_DWORDS = GT_MEXP_GROUP * GT_EXP_TAB_DWORDS;        // per lane: 4 tables x 16 rows x 256 bytes
constexpr size_t GT_MEXP_TAB_BYTES = 2 * (size_t)GT_MEXP_TAB_DWORDS * sizeof(int32_t);      // per piece: both lanes of the pair
// lane pairs that fill the chip: 256 CUs x 4 SIMDs x 2 waves x 32 pairs; a product-only piece has at least 8 factors on average
constexpr SegRedShape GT_MEXP_SHAPE{65536, GT_MEXP_GROUP, 8};

// prod_{i < cnt} base(i)^{k_i}, digit(i, w) = window w (0 = lowest) of k_i.  Every lane of the wavefront must call it (x.all); the
// trip counts are the wavefront's longest, pairs with fewer factors ride along on one = row 0 of a table that holds nothing else.
template <class X, class Base, class Digit>
GPBC_INLINE F6 f12p_multi_exp(const X &x, size_t cnt, Base base, Digit digit, int32_t *tab) {
    F6 acc = f12p_one(x);
    for (size_t g0 = 0; !x.all(g0 >= cnt); g0 += GT_MEXP_GROUP) {
        const int nf = g0 >= cnt ? 0 : cnt - g0 < (size_t)GT_MEXP_GROUP ? (int)(cnt - g0) : GT_MEXP_GROUP;
        int nfw = 1;
        while (nfw < GT_MEXP_GROUP && !x.all(nf <= nfw)) nfw++;
        bool cyc = true;
#pragma unroll 1
        for (int j = 0; j < nfw; j++) {
            int32_t *t = tab + j * GT_EXP_TAB_DWORDS;
            F6 cur = f12p_one(x);
            f6_row_store(t, cur);
            if (j < nf) {                                                   // (pairs diverge here at most; nothing below asks the wavefront)
                const F6 b = base(g0 + j);
                cyc = cyc && f12p_is_cyclotomic(x, b);
                cur = b;
                f6_row_store(t + GT_EXP_ROW_DWORDS, cur);
#pragma unroll 1
                for (int i = 2; i < 16; i++) { cur = f12p_mul(x, cur, b); f6_row_store(t + i * GT_EXP_ROW_DWORDS, cur); }
            }
        }
        // f12p_exp256's rule, per group: Granger-Scott squarings when every base of the wavefront's groups is cyclotomic
        cyc = x.all(cyc);
        auto row = [&](int j, int w) { return f6_row_load(tab + j * GT_EXP_TAB_DWORDS + (j < nf ? digit(g0 + j, w) : 0) * GT_EXP_ROW_DWORDS); };
        F6 r = row(0, 63);
#pragma unroll 1
        for (int j = 1; j < nfw; j++) r = f12p_mul(x, r, row(j, 63));
#pragma unroll 1
        for (int w = 62; w >= 0; w--) {
            if (cyc) { bool flipped = false; r = f12p_cyclo_sqr_run(x, r, 4, flipped); }
            else for (int s = 0; s < 4; s++) r = f6_reduce(f12p_sqr(x, r));
#pragma unroll 1
            for (int j = 0; j < nfw; j++) r = f12p_mul(x, r, row(j, w));    // several products in a row, no squaring between
        }
        if (g0 == 0) acc = r;
        else f12p_mul_to(x, acc, acc, r);
    }
    return acc;
}
// prod_{i < cnt} base(i): no exponents, no squarings, no tables
template <class X, class Base> GPBC_INLINE F6 f12p_product(const X &x, size_t cnt, Base base) {
    F6 acc = f12p_one(x);
    for (size_t i = 0; !x.all(i >= cnt); i++)
        if (i < cnt) acc = f12p_mul(x, acc, base(i));
    return acc;
}

}  // namespace gpbc
#endif
