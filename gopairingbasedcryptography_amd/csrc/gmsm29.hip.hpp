// Segmented multi-scalar multiplication in G1 / G2 on one lane: out = sum_i [k_i] P_i over a run of terms, every term with the
// semantics of scalar_mul29_best (any 256-bit scalar acting mod r, the all-zero point = infinity) and ONE chain of doublings for
// GMSM_GROUP terms (Straus interleaving): the terms are taken four at a time, each with the 16-row table of its own endomorphism
// split (glv_table29 / gls_table29), and a window costs its doublings once plus one mixed addition per term.  Paper count per term
// in Fp products: G1 910 / 4 + 715 + 200 + ~35 for the common curve = ~1 180 where the single-term loop spends ~1 825, G2
// 460 / 4 + 730 + 300 + ~35 = ~1 180 (Fp2 products) where it spends ~1 490.  The common curve costs two products per row and five
// per term for f_j, f_j^2, f_j^3 and the running products: ~35 either way.
//
// Common curve.  A term's table sits on the isomorphic curve y^2 = x^3 + b W_j^6, W_j the product of that table's Z's.  Terms that
// share an accumulator must sit on ONE curve, W = prod_j W_j: every row of term j is multiplied by f_j^2 (x) and f_j^3 (y),
// f_j = W / W_j from prefix / suffix products (no inversion), and the group's Jacobian result gets its Z multiplied by W once.  A
// group of one term skips the step and is scalar_mul29_best's loop.
//
// A lane's block of the workspace (gmsm_lane_dwords<F>() int32, a whole number of 128-byte rows; the rows are read and written as
// 128-bit TabQuads, so the workspace must be 16-byte aligned — the entries refuse one that is not): GMSM_GROUP tables in the TabQuad row layout of
// curve29.hip.hpp (2 KB per term for G1, 4 KB for G2; row 0 of a table, which no digit selects, holds W_j and its prefix product
// while the group is set up), then GMSM_DIGIT_DWORDS window words: word w holds the table index of every term of the group for
// window w, four bits per term; then the piece's Jacobian accumulator.  The accumulator lives there and not in registers: it is not
// needed while a group's loop runs (27 / 54 registers less under the loop).  It is also a work-around: with the accumulator in
// registers the gfx950 build of the G2 kernel gave wrong sums for lanes whose piece had fewer groups than another lane of their
// wavefront (G and G + 1 terms side by side; DESIGN.md 15 has what was seen) — a suspected compiler problem that was not reduced
// further; every lane now reads its own result back from memory after the loop.  The next group overwrites the tables and the
// window words, so the block is a lane's whole footprint whatever the run's length.
// The work is cut by csrc/segred29.hip.hpp with GMSM_SHAPE (one lane per piece): the kernels (csrc/gpbc_gmsm.hip) and the host interval
// harness (tools/bounds_check.cpp, hc_multi_scalar_mul) run one plan.
#ifndef GPBC_GMSM29_HIP_HPP
#define GPBC_GMSM29_HIP_HPP
#include "curve29.hip.hpp"
#include "segred29.hip.hpp"

namespace gpbc {

#ifndef GMSM_GROUP
#define GMSM_GROUP 4                                                         // terms that share a chain of doublings (at most 8: four index bits per term in a 32-bit window word)
#endif
static_assert(GMSM_GROUP >= 1 && GMSM_GROUP <= 8, "a window word holds four index bits for each of at most 8 terms");
constexpr int GMSM_DIGIT_DWORDS = 128;                                       // 80 two-bit windows of a 160-bit GLV half / 96 bits of a GLS quarter, padded to a whole number of 128-byte rows
// lanes that fill the chip: 256 CUs x 4 SIMDs x 2 waves x 64 lanes; a piece of a plain sum has at least 8 points on average
constexpr SegRedShape GMSM_SHAPE{131072, GMSM_GROUP, 8};
template <class F> constexpr int gmsm_acc_dwords() { return (int)((sizeof(JacP<F>) + 127) / 128) * 32; }   // the piece's accumulator, whole 128-byte rows
template <class F> constexpr int gmsm_lane_dwords() { return GMSM_GROUP * glv_table_dwords<F>() + GMSM_DIGIT_DWORDS + gmsm_acc_dwords<F>(); }

// ---- one term: split, table, window indices.  Returns the term's highest window (-1: the term contributes nothing — a base at
// infinity or a scalar = 0 mod r — and has no table; its indices stay 0).  slot = the term's position in the group.
GPBC_INLINE int gmsm_term(int32_t *tab, uint32_t *dig, int slot, Fe &W, const AffP<Fe> &base, const uint32_t k[8]) {
    GlvSplit s;
    glv_split(s, k);
    int top = 159;
    while (top >= 0 && !(((s.k1[top >> 5] | s.k2[top >> 5]) >> (top & 31)) & 1)) top--;
    if (base.inf || top < 0) return -1;
    AffP<Fe> p1{base.x, s.neg1 ? g_neg(base.y) : base.y, false};
    AffP<Fe> p2{glv_phi_x(base.x), s.neg2 ? g_neg(base.y) : base.y, false};
    glv_table29<Fe>(tab, W, p1, p2, s.neg1 != s.neg2);
#pragma unroll
    for (int wd = 0; wd < 5; wd++) {
        const uint32_t a = s.k1[wd], b = s.k2[wd];
        if (!(a | b)) continue;
        for (int t = 0; t < 16; t++) {                                      // index = 4 d1 + d2 of the two-bit window, as scalar_mul29_jac reads it
            const uint32_t idx = 4 * ((a >> (2 * t)) & 3) + ((b >> (2 * t)) & 3);
            if (idx) dig[wd * 16 + t] |= idx << (4 * slot);
        }
    }
    return top >> 1;
}
GPBC_INLINE int gmsm_term(int32_t *tab, uint32_t *dig, int slot, F2 &W, const AffP<F2> &base, const uint32_t k[8]) {
    GlsSplit s;
    gls_split(s, k);
    int top = 95;
    while (top >= 0 && !(((s.k[0][top >> 5] | s.k[1][top >> 5] | s.k[2][top >> 5] | s.k[3][top >> 5]) >> (top & 31)) & 1)) top--;
    if (base.inf || top < 0) return -1;
    AffP<F2> P[4];
    P[0] = AffP<F2>{base.x, s.neg[0] ? f2_neg(base.y) : base.y, false};
    for (int i = 1; i < 4; i++) {
        const bool cj = i & 1;
        F2 y = f2_mul(cj ? f2_conj(base.y) : base.y, gamma29(i, 3));
        P[i] = AffP<F2>{f2_mul(cj ? f2_conj(base.x) : base.x, gamma29(i, 2)), s.neg[i] ? f2_neg(y) : y, false};
    }
    gls_table29(tab, W, P);
#pragma unroll
    for (int wd = 0; wd < 3; wd++) {
        const uint32_t a = s.k[0][wd], b = s.k[1][wd], c = s.k[2][wd], d = s.k[3][wd];
        if (!(a | b | c | d)) continue;
        for (int t = 0; t < 32; t++) {                                      // index = b0 + 2 b1 + 4 b2 + 8 b3 of the bit, as scalar_mul29_gls reads it
            const uint32_t idx = ((a >> t) & 1) | (((b >> t) & 1) << 1) | (((c >> t) & 1) << 2) | (((d >> t) & 1) << 3);
            if (idx) dig[wd * 32 + t] |= idx << (4 * slot);
        }
    }
    return top;
}
template <class F> struct GmsmLoop;
template <> struct GmsmLoop<Fe> { static constexpr int DOUBLINGS = 2, WINDOWS = 80; };     // two-bit windows over the GLV halves
template <> struct GmsmLoop<F2> { static constexpr int DOUBLINGS = 1, WINDOWS = 96; };     // one bit of each of the four GLS quarters

// W_j and a second value in row 0 of a term's table (the row no index selects)
template <class F> GPBC_INLINE void gmsm_w_put(int32_t *tab, const F &w, const F &pre) { tab_store(tab, 0, AffP<F>{w, pre, false}); }
template <class F> GPBC_INLINE void gmsm_w_get(const int32_t *tab, F &w, F &pre) {
    AffP<F> t;
    tab_load(tab, 0, t);
    w = t.x; pre = t.y;
}

// sum_{i < cnt} [k_i] base(i) as a Jacobian point; scalar(i, k) fills the eight words of k_i; ws = this lane's block
template <class F, class Base, class Scalar> GPBC_INLINE JacP<F> gmsm_lane(size_t cnt, Base base, Scalar scalar, int32_t *ws) {
    constexpr int TD = glv_table_dwords<F>();
    uint32_t *dig = reinterpret_cast<uint32_t *>(ws + GMSM_GROUP * TD);
    JacP<F> *sum = reinterpret_cast<JacP<F> *>(ws + GMSM_GROUP * TD + GMSM_DIGIT_DWORDS);
    F one;
    g_set_one(one);
    {
        JacP<F> inf;
        jac_set_inf(inf);
        *sum = inf;
    }
    for (size_t g0 = 0; g0 < cnt; g0 += GMSM_GROUP) {
        const int nf = cnt - g0 < (size_t)GMSM_GROUP ? (int)(cnt - g0) : GMSM_GROUP;
        for (int w = 0; w < GmsmLoop<F>::WINDOWS; w++) dig[w] = 0;
        int top = -1;
        uint32_t have = 0;                                                  // bit j: term j has a table
        F W = one;                                                          // the product of the W_j so far
#pragma unroll 1
        for (int j = 0; j < nf; j++) {
            uint32_t k[8];
            scalar(g0 + j, k);
            F Wj = one;
            const int t = gmsm_term(ws + j * TD, dig, j, Wj, base(g0 + j), k);
            if (t >= 0) have |= 1u << j;
            if (t > top) top = t;
            if (nf > 1) { gmsm_w_put<F>(ws + j * TD, Wj, W); W = g_mul(W, Wj); }        // row 0: W_j and the prefix product before it
            else W = Wj;
        }
        if (top < 0) continue;                                              // nothing but infinity and zero scalars in this group
        if (nf > 1) {
            // every table onto the curve of W = prod W_j: row (x, y) of term j becomes (x f^2, y f^3), f = W / W_j = pre_j suf_j
            F run = one;
#pragma unroll 1
            for (int j = nf - 1; j >= 0; j--) {
                F wj, pre;
                gmsm_w_get<F>(ws + j * TD, wj, pre);
                const F f = g_mul(pre, run);
                run = g_mul(run, wj);
                if (!((have >> j) & 1)) continue;
                const F f2 = g_sqr(f), f3 = g_mul(f2, f);
#pragma unroll 1
                for (int r = 1; r < 16; r++) {
                    AffP<F> e;
                    tab_load(ws + j * TD, r, e);
                    tab_store(ws + j * TD, r, AffP<F>{g_mul(e.x, f2), g_mul(e.y, f3), false});
                }
            }
        }
        // the joint loop: the window's doublings once, then one mixed addition per term whose index is not 0.  A term's row is
        // requested one step ahead (the first before the doublings, as scalar_mul29_jac does): its latency passes behind the step.
        JacP<F> acc;
        jac_set_inf(acc);
#pragma unroll 1
        for (int w = top; w >= 0; w--) {
            const uint32_t d = dig[w];
            int idx = (int)(d & 15);
            AffP<F> t;
            tab_load(ws, idx, t);
            for (int s = 0; s < GmsmLoop<F>::DOUBLINGS; s++) jac_dbl(acc, acc);
#pragma unroll 1
            for (int j = 0; j < nf; j++) {
                const int jn = j + 1 < nf ? j + 1 : j;
                const int nidx = (int)((d >> (4 * jn)) & 15);
                AffP<F> nx;
                tab_load(ws + jn * TD, nidx, nx);
                if (idx) jac_add_mixed(acc, acc, t);                        // equal or opposite to the accumulator: doubling / infinity, handled there
                t = nx; idx = nidx;
            }
        }
        if (!acc.inf) acc.z = g_mul(acc.z, W);                              // back from the curve scaled by W
        JacP<F> s = *sum;
        jac_add(s, s, acc);
        *sum = s;
    }
    return *sum;
}
// sum_{i < cnt} base(i): no scalars, no tables, no doublings (also the fold of the piece values between levels)
template <class F, class Base> GPBC_INLINE JacP<F> gmsm_sum_lane(size_t cnt, Base base) {
    JacP<F> acc;
    jac_set_inf(acc);
    for (size_t i = 0; i < cnt; i++) jac_add_mixed(acc, acc, base(i));
    return acc;
}

}  // namespace gpbc
#endif
