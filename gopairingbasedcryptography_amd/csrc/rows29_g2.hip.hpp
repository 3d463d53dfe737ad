// Per-row shared-base scalar multiplication in G2 from row tables, for gfx950: the G2 side of csrc/rows29.hip.hpp.  The consumer is the key
// generation of BSW07 (Dj[u, a] = [r_u] g2 + [rj_ua] H2(a), cpabe/bsw07/bsw07_cpabe.go:97-131: one hashed point per attribute, a row of
// per-user scalars per point).
//
// G2 rows from ROWS_G2_TABLE_MIN scalars on get a small table per base over the four-dimensional GLS split of curve29.hip.hpp:
//   geometry   gls_split gives k = sum +-k_i mu^i with mu = 6 u^2 the eigenvalue of psi and every |k_i| < 2^66 (the Babai residual is at
//              most the column sums of |B|, max (8 u + 3)(1 + eps); tests/test_device_math_bounds.py holds it on 20 000 scalars), so a
//              quarter fits 17 windows of 4 bits, the top one holding two.  Entry (w, d) = [d 16^w] P, d = 1 .. 15, affine, in the 256-byte
//              row layout of TabLayout<F2> (tab_store / tab_load): all 17 x 15 = 255 rows = 65 280 B a base (window 16 keeps its 15 rows: a
//              quarter up to 2^68 - 1 is served, and every window is addressed alike).  Only P has rows: the images under psi are never stored.
//   build (a)  one lane per base: 64 doublings, the 17 window bases 16^w P kept and brought to affine with one inversion, written to a
//              4 352-byte block per base; the base's infinity flag.  Run ONCE for up to ROWS_G2_GROUP_BASES bases ahead of their passes.
//   build (b)  one lane per (base, window): 2B .. 15B from the window base B by one doubling and 13 mixed additions, one inversion for
//              the 14; B and they are the window's 15 rows.
//   evaluation one lane per output: gls_split, then Horner over the quarters with psi applied to the ACCUMULATOR,
//              acc = S3; acc = psi(acc) + S2; acc = psi(acc) + S1; acc = psi(acc) + S0, S_i = the <= 17 looked-up rows of quarter i, each
//              with y negated when neg[i]: three psi (six Fp2 products) and at most 68 mixed additions, no doublings; digit 0 is skipped.
//              On Jacobian coordinates psi is (conj X gamma_2, conj Y gamma_3, conj Z) with the constants scalar_mul29_gls takes from
//              gamma29; an accumulator at infinity stays there.
// jac_add_mixed is the complete law, so the doubling inside a chain, a cancellation and the restart after it are its exceptional branches
// (the contract of fbindex29.hip.hpp), and every scalar up to 2^256 - 1 comes out as [k mod r] P for P in the order-r subgroup (psi acts
// as [mu] there only; scalar_mul29_gls presumes the same).
// The lane functions are shared with the host harness (tools/rows_g2_check.cpp); none of them uses blockIdx.
#ifndef GPBC_ROWS29_G2_HIP_HPP
#define GPBC_ROWS29_G2_HIP_HPP
#include "curve29.hip.hpp"

namespace gpbc {

constexpr int ROWS_G2_WINDOWS = 17, ROWS_G2_DIGITS = 15, ROWS_G2_ENTRIES = ROWS_G2_WINDOWS * ROWS_G2_DIGITS, ROWS_G2_QUARTERS = 4;
constexpr size_t ROWS_G2_ENTRY_DWORDS = (size_t)TabLayout<F2>::ENTRY_DWORDS;
constexpr size_t ROWS_G2_TABLE_BYTES = (size_t)ROWS_G2_ENTRIES * ROWS_G2_ENTRY_DWORDS * sizeof(int32_t);      // per base: 65 280
// Scalars per base from which a G2 row takes the tables: the smallest measured row length from which the tables beat the table-free
// kernel at every larger one by more than the run-to-run spread (MI355X, 2^20 outputs, profiles/shared_base_rows_g2.json: 1.47 x slower
// at m = 8, 9.5 % faster at 16, 31 % at 32, 58 % at 4 096; spread 1.0 %).  The build measures at about 12 evaluations per base.
constexpr size_t ROWS_G2_TABLE_MIN = 16;
// Bases are worked off in passes: a pass has about ROWS_G2_PASS_OUTPUTS outputs where the call has them, and its tables stay under
// ROWS_G2_TABLE_CAP bytes.
constexpr size_t ROWS_G2_PASS_OUTPUTS = (size_t)1 << 18, ROWS_G2_TABLE_CAP = (size_t)1 << 30;
constexpr size_t ROWS_G2_WB_BYTES = (size_t)ROWS_G2_WINDOWS * ROWS_G2_ENTRY_DWORDS * sizeof(int32_t);         // window bases per base: 4 352
constexpr size_t ROWS_G2_GROUP_BASES = (size_t)1 << 16;                                                      // bases per launch of build (a): 272 MiB of window bases
inline size_t rows_g2_pass_bases(size_t nbase, size_t m) {
    size_t p = ROWS_G2_PASS_OUTPUTS / m, cap = ROWS_G2_TABLE_CAP / ROWS_G2_TABLE_BYTES;
    if (p > cap) p = cap;
    if (p < 1) p = 1;
    return p < nbase ? p : nbase;
}

GPBC_INLINE int32_t *rows_g2_entry(int32_t *table, int w, int d) { return table + (size_t)(w * ROWS_G2_DIGITS + d - 1) * ROWS_G2_ENTRY_DWORDS; }
GPBC_INLINE const int32_t *rows_g2_entry(const int32_t *table, int w, int d) { return table + (size_t)(w * ROWS_G2_DIGITS + d - 1) * ROWS_G2_ENTRY_DWORDS; }

// build (a): `wb` = this base's 17 rows of window bases (row w = 16^w P), *inf = its flag.  A base at infinity writes the flag and no
// row; (b) and the evaluation read the flag before any row.
GPBC_INLINE void rows_g2_build_a_lane(const AffP<F2> &base, int32_t *wb, uint8_t *inf) {
    *inf = base.inf ? 1 : 0;
    if (base.inf) return;
    JacP<F2> W[ROWS_G2_WINDOWS];
    W[0].x = base.x; W[0].y = base.y; g_set_one(W[0].z); W[0].inf = false;
    for (int w = 1; w < ROWS_G2_WINDOWS; w++) {
        JacP<F2> t;
        jac_dbl(t, W[w - 1]);
        jac_dbl(t, t);
        jac_dbl(t, t);
        jac_dbl(W[w], t);
    }
    AffP<F2> A[ROWS_G2_WINDOWS];
    jac_to_affine_batch<F2, ROWS_G2_WINDOWS>(A, W);
    for (int w = 0; w < ROWS_G2_WINDOWS; w++) tab_store(wb, w, A[w]);
}

// build (b): window w of the base whose window bases are `wb` (build (a), an earlier launch on the same stream) into its rows `table`
GPBC_INLINE void rows_g2_build_b_lane(const int32_t *wb, int32_t *table, const uint8_t *inf, int w) {
    if (*inf) return;
    AffP<F2> B;
    tab_load(wb, w, B);
    JacP<F2> M[ROWS_G2_DIGITS - 1];                            // 2B .. 15B
    JacP<F2> b1;
    b1.x = B.x; b1.y = B.y; g_set_one(b1.z); b1.inf = false;
    jac_dbl(M[0], b1);
    for (int d = 1; d < ROWS_G2_DIGITS - 1; d++) jac_add_mixed(M[d], M[d - 1], B);
    AffP<F2> A[ROWS_G2_DIGITS - 1];
    jac_to_affine_batch<F2, ROWS_G2_DIGITS - 1>(A, M);
    tab_store(rows_g2_entry(table, w, 1), 0, B);
    for (int d = 0; d < ROWS_G2_DIGITS - 1; d++) tab_store(rows_g2_entry(table, w, d + 2), 0, A[d]);
}

// psi on a Jacobian point: (conj X gamma_(1,2), conj Y gamma_(1,3), conj Z); infinity stays.  Two Fp2 products.
GPBC_INLINE void rows_g2_psi(JacP<F2> &p) {
    if (p.inf) return;
    p.x = f2_mul(f2_conj(p.x), gamma29(1, 2));
    p.y = f2_mul(f2_conj(p.y), gamma29(1, 3));
    p.z = f2_norm(f2_conj(p.z));
}

// Evaluation over a split that is GIVEN: sum_i +-k_i mu^i P from the low 68 bits of the four magnitudes (the harness runs it on sign
// patterns and digits gls_split never returns).  Step t = 17 (3 - i) + w: window w of quarter i, quarter 3 first; entering a later
// quarter the accumulator goes through psi once.  The next row is requested before the addition so that its latency passes behind it.
GPBC_INLINE void rows_g2_eval_split(JacP<F2> &acc, const int32_t *table, bool base_inf, const GlsSplit &s) {
    jac_set_inf(acc);
    if (base_inf) return;
    constexpr int STEPS = ROWS_G2_QUARTERS * ROWS_G2_WINDOWS;
    auto digit = [&](int t) { const int i = 3 - t / ROWS_G2_WINDOWS, w = t % ROWS_G2_WINDOWS; return (int)((s.k[i][w >> 3] >> (4 * (w & 7))) & 15u); };
    int d = digit(0);
    AffP<F2> e;
    tab_load(rows_g2_entry(table, 0, d ? d : 1), 0, e);
    for (int t = 0; t < STEPS; t++) {
        const int tn = t + 1 < STEPS ? t + 1 : 0;
        const int dn = t + 1 < STEPS ? digit(tn) : 0;
        AffP<F2> en;
        tab_load(rows_g2_entry(table, tn % ROWS_G2_WINDOWS, dn ? dn : 1), 0, en);
        if (t && t % ROWS_G2_WINDOWS == 0) rows_g2_psi(acc);
        if (d) {
            if (s.neg[3 - t / ROWS_G2_WINDOWS]) e.y = f2_neg(e.y);
            jac_add_mixed(acc, acc, e);
        }
        e = en; d = dn;
    }
}
// *wide is set when a quarter does not fit the 17 windows (never: the harness checks it over its whole case table); the result is then
// the multiple for the low 68 bits of the quarters only.
GPBC_INLINE void rows_g2_eval_lane(JacP<F2> &acc, const int32_t *table, bool base_inf, const uint32_t k[8], bool *wide = nullptr) {
    GlsSplit s;
    gls_split(s, k);
    if (wide) *wide = ((s.k[0][2] | s.k[1][2] | s.k[2][2] | s.k[3][2]) >> 4) != 0;
    rows_g2_eval_split(acc, table, base_inf, s);
}

}  // namespace gpbc
#endif
