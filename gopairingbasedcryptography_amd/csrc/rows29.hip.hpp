// Per-row shared-base scalar multiplication for gfx950: out[j m + i] = [k_(j m + i)] base_j, one base per ROW of m scalars.  The key
// generation of LW11 has this shape (K_(i,GID) = g1^alpha_i + [y_i] H(GID), dabe/lw11_dabe.go:90-107: one hashed point per user, a row of
// authority secrets per point), and so has every loop that raises a per-user or per-message point to a list of secrets.  It is the shape
// between "one base for all" (the transient 8-bit table of gpbc_curve.hip, 1 MB built by 8 160 scalar multiplications) and "a base each"
// (scalar_mul29: a GLV table per output, ~130 doublings and ~65 additions).
//
// G1 rows from ROWS_TABLE_MIN scalars on get a SMALL table per base, built by a chain, used for the row and thrown away:
//   geometry   the GLV halves |k1|, |k2| of a scalar are below 2^128 (see rows_eval_lane), 32 windows of 4 bits each; entry (w, d) =
//              [d 16^w] P, d = 1 .. 15, affine, in the 128-byte row layout of curve29.hip.hpp (tab_store / tab_load): 480 rows = 60 KiB a base.
//              The phi(P) half needs no rows of its own: phi is a group endomorphism, so [d 16^w] phi(P) = (beta x, y) of entry (w, d).
//   build (a)  one lane per base: 124 doublings, the 32 window bases 16^w P kept and brought to affine with one inversion, written to a
//              4 KiB block per base; the base's infinity flag.  A lane walks ~1 600 dependent products whatever the batch, so (a) runs
//              ONCE for up to ROWS_GROUP_BASES bases ahead of their passes, not once a pass.
//   build (b)  one lane per (base, window): 2B .. 15B from the window base B by one doubling and 13 mixed additions, one inversion for
//              the 14; B and they are the window's 15 rows.
//   evaluation one lane per output: glv_split, then 32 + 32 look-ups and mixed additions, no doublings; digit 0 is skipped.
// jac_add_mixed is the complete law, so the doubling inside a chain, a cancellation and the restart after it are its exceptional branches
// (the contract of fbindex29.hip.hpp), and every scalar up to 2^256 - 1 comes out as [k mod r] P.
// Everything else (G1 and G2 rows below their crossovers) takes rows_free_lane: scalar_mul29_best as k_g1 / g2_scalar_mul use it, lane i
// on base i / m.  The G2 table form — the four-dimensional GLS split, 17 windows per quarter, psi on the accumulator — is
// csrc/rows29_g2.hip.hpp with kernels of its own in csrc/gpbc_rows_g2.hip; scalar_mul_rows_dev sends G2 rows of ROWS_G2_TABLE_MIN
// scalars and more there.  The ROWS_* constants below are G1's; G2 has ROWS_G2_*.
// The lane functions are shared with the host harness (tools/rows_check.cpp); none of them uses blockIdx.
#ifndef GPBC_ROWS29_HIP_HPP
#define GPBC_ROWS29_HIP_HPP
#include "curve29.hip.hpp"

namespace gpbc {

constexpr int ROWS_WINDOWS = 32, ROWS_DIGITS = 15, ROWS_ENTRIES = ROWS_WINDOWS * ROWS_DIGITS;
constexpr size_t ROWS_ENTRY_DWORDS = (size_t)TabLayout<Fe>::ENTRY_DWORDS;
constexpr size_t ROWS_TABLE_BYTES = (size_t)ROWS_ENTRIES * ROWS_ENTRY_DWORDS * sizeof(int32_t);      // per base: 61 440
// Scalars per base from which a G1 row takes the tables: the smallest measured row length from which the tables won at every larger
// one (MI355X, 2^20 outputs, profiles/shared_base_rows.json: 4.8 % slower than one base per scalar at m = 16, 23 % faster at 32, 46 %
// at 4 096).  Operation counts had put the break-even near 8; the build measures at about 15 evaluations per base, not 12.
constexpr size_t ROWS_TABLE_MIN = 32;
// Bases are worked off in passes: a pass has about ROWS_PASS_OUTPUTS outputs where the call has them, and its tables stay under
// ROWS_TABLE_CAP bytes.
constexpr size_t ROWS_PASS_OUTPUTS = (size_t)1 << 18, ROWS_TABLE_CAP = (size_t)1 << 30;
constexpr size_t ROWS_WB_BYTES = (size_t)ROWS_WINDOWS * ROWS_ENTRY_DWORDS * sizeof(int32_t);         // window bases per base: 4 096
constexpr size_t ROWS_GROUP_BASES = (size_t)1 << 16;                                                // bases per launch of build (a): 256 MiB of window bases
inline size_t rows_pass_bases(size_t nbase, size_t m) {
    size_t p = ROWS_PASS_OUTPUTS / m, cap = ROWS_TABLE_CAP / ROWS_TABLE_BYTES;
    if (p > cap) p = cap;
    if (p < 1) p = 1;
    return p < nbase ? p : nbase;
}

GPBC_INLINE int32_t *rows_entry(int32_t *table, int w, int d) { return table + (size_t)(w * ROWS_DIGITS + d - 1) * ROWS_ENTRY_DWORDS; }
GPBC_INLINE const int32_t *rows_entry(const int32_t *table, int w, int d) { return table + (size_t)(w * ROWS_DIGITS + d - 1) * ROWS_ENTRY_DWORDS; }

// build (a): `wb` = this base's 32 rows of window bases (row w = 16^w P), *inf = its flag.  A base at infinity writes the flag and no
// row; (b) and the evaluation read the flag before any row.
GPBC_INLINE void rows_build_a_lane(const AffP<Fe> &base, int32_t *wb, uint8_t *inf) {
    *inf = base.inf ? 1 : 0;
    if (base.inf) return;
    JacP<Fe> W[ROWS_WINDOWS];
    W[0].x = base.x; W[0].y = base.y; g_set_one(W[0].z); W[0].inf = false;
    for (int w = 1; w < ROWS_WINDOWS; w++) {
        JacP<Fe> t;
        jac_dbl(t, W[w - 1]);
        jac_dbl(t, t);
        jac_dbl(t, t);
        jac_dbl(W[w], t);
    }
    AffP<Fe> A[ROWS_WINDOWS];
    jac_to_affine_batch<Fe, ROWS_WINDOWS>(A, W);
    for (int w = 0; w < ROWS_WINDOWS; w++) tab_store(wb, w, A[w]);
}

// build (b): window w of the base whose window bases are `wb` (build (a), an earlier launch on the same stream) into its rows `table`
GPBC_INLINE void rows_build_b_lane(const int32_t *wb, int32_t *table, const uint8_t *inf, int w) {
    if (*inf) return;
    AffP<Fe> B;
    tab_load(wb, w, B);
    JacP<Fe> M[ROWS_DIGITS - 1];                               // 2B .. 15B
    JacP<Fe> b1;
    b1.x = B.x; b1.y = B.y; g_set_one(b1.z); b1.inf = false;
    jac_dbl(M[0], b1);
    for (int d = 1; d < ROWS_DIGITS - 1; d++) jac_add_mixed(M[d], M[d - 1], B);
    AffP<Fe> A[ROWS_DIGITS - 1];
    jac_to_affine_batch<Fe, ROWS_DIGITS - 1>(A, M);
    tab_store(rows_entry(table, w, 1), 0, B);
    for (int d = 0; d < ROWS_DIGITS - 1; d++) tab_store(rows_entry(table, w, d + 2), 0, A[d]);
}

// Evaluation: [k] P from P's rows.  The halves fit the 32 windows: with c_i = floor(k g_i / 2^256) the split leaves
// k1 = e1 a1 + e2 a2, k2 = e2 b2 - e1 |b1| with -0.2 < e_i < 1.2 (the floor, and g_i off 2^256 b / r by less than 1), a1 = b2 < 2^64
// and a2, |b1| < 2^127, so |k1|, |k2| < 1.2 (2^64 + 2^127) < 2^128; word 4 of a half is zero.  *wide is set when it is not (never: the
// harness checks it over its whole case table) and the result is then [k] P for the low 128 bits of the halves only.
// Step t = 2 w + h: window w of half h.  The next row is requested before the addition so that its latency passes behind it.
// rows_eval_split is the walk over a split that is given: +-k1 P +- k2 phi(P) from the low 128 bits of the halves (the harness runs it on
// splits that glv_split never produces — it returns k1 >= 0 only — so that every sign and every window of both halves is checked).
GPBC_INLINE void rows_eval_split(JacP<Fe> &acc, const int32_t *table, bool base_inf, const GlvSplit &s) {
    jac_set_inf(acc);
    if (base_inf) return;
    auto digit = [&](int t) { const int w = t >> 1; return (int)((((t & 1) ? s.k2[w >> 3] : s.k1[w >> 3]) >> (4 * (w & 7))) & 15u); };
    int d = digit(0);
    AffP<Fe> e;
    tab_load(rows_entry(table, 0, d ? d : 1), 0, e);
    for (int t = 0; t < 2 * ROWS_WINDOWS; t++) {
        const int dn = t + 1 < 2 * ROWS_WINDOWS ? digit(t + 1) : 0;
        AffP<Fe> en;
        tab_load(rows_entry(table, t + 1 < 2 * ROWS_WINDOWS ? (t + 1) >> 1 : 0, dn ? dn : 1), 0, en);
        if (d) {
            const bool h = (t & 1) != 0;
            if (h) e.x = glv_phi_x(e.x);
            if (h ? s.neg2 : s.neg1) e.y = g_neg(e.y);
            jac_add_mixed(acc, acc, e);
        }
        e = en; d = dn;
    }
}
GPBC_INLINE void rows_eval_lane(JacP<Fe> &acc, const int32_t *table, bool base_inf, const uint32_t k[8], bool *wide = nullptr) {
    GlvSplit s;
    glv_split(s, k);
    if (wide) *wide = (s.k1[4] | s.k2[4]) != 0;
    rows_eval_split(acc, table, base_inf, s);
}

// The table-free row lane: the multiplication of k_g1 / g2_scalar_mul on the row's base; tab = this lane's glv_table_dwords<F>() int32
template <class F> GPBC_INLINE void rows_free_lane(AffP<F> &out, const AffP<F> &base, const uint32_t k[8], int32_t *tab) {
    JacP<F> res[1];                                            // the body of k_g1 / g2_scalar_mul at SMUL_K = 1, statement for statement: the
    scalar_mul29_best(res[0], base, k, tab);                   // plain jac_to_affine here made the G1 kernel spill more and run 7 % slower
    AffP<F> aff[1];
    jac_to_affine_batch<F, 1>(aff, res);
    out = aff[0];
}

}  // namespace gpbc
#endif
