// Opening proofs over the fixed-base window tables of csrc/gpbc_curve.hip for gfx950, with the quotient's coefficients made in the lane that
// adds their terms: pi_i = sum_{c < m} q_(i,c) [tau^c], q_i(X) = f(X) / (X - id_i), for every identity of a batch of m <= B identities
// (bibe/gwww25_bibe/gwww25_bibe.go:211-228 in G2, bibe/afp25_bibe/afp25_bibe.go:369-393 in G1).  The lane function and the geometry of a
// call live here so that the kernels (k_g1/g2_fb_openings in csrc/gpbc_openings.hip) and the host harness (tools/bounds_check.cpp:
// hc_fb_openings) run the same code; neither uses blockIdx.
//
// Synthetic division walks from the top: q_(m-1) = f_m, q_(c-1) = f_c + id q_c (fr_poly_horner_step, canonical as it falls out), and the
// step after q_0 leaves the remainder f(id).  A lane owns the bases [c_lo, c_hi) of one identity: it walks the steps above c_hi with no
// group work, then per base one step, the canonical words of the coefficient, and what fb_msm_lane does with a scalar — 32 windows of 8
// bits, per non-zero digit one table row and one mixed addition.  jac_add_mixed is the complete law, so a sum that passes through infinity
// (tau itself among the identities makes every other opening of the batch the point at infinity) comes out as the group says.
//
// The lane whose chunk starts at base 0 reaches the constant term and decides ok: the remainder is zero AND q(id) is not — q(id) = f'(id),
// evaluated by a second Horner chain over the coefficients as they fall out, is zero exactly when id is a root more than once, which is the
// reference's "exactly one identity removed" rule (gwww25_bibe.go:214-223, afp25_bibe.go:371-381) for a batch with a repeated identity.
#ifndef GPBC_OPENINGS29_HIP_HPP
#define GPBC_OPENINGS29_HIP_HPP
#include "curve29.hip.hpp"
#include "fr29.hip.hpp"

namespace gpbc {

constexpr int OPN_WINDOWS = 32, OPN_DIGITS = 255, OPN_ENTRIES = OPN_WINDOWS * OPN_DIGITS;     // the table geometry of gpbc_curve.hip (FB_*)
constexpr int OPN_WAVE = 64;
constexpr uint32_t OPN_SMALL_M = 256, OPN_MAX_M = FR_POLY_MAX_B;                               // the two LDS instances of the staging

// One wave's identities: `rows` <= 64 consecutive identities, the first of them identity id0 of the call, all of segment `seg`, which holds
// m of them.  Built on the host from the segment table (opn_blocks); an empty segment has no block.
struct OpnBlock { uint64_t id0; uint32_t seg, m, rows, pad; };

// bases per lane: enough lanes to fill the chip before a lane takes more than one base, at most 16 — the rule of fb_shape (gpbc_curve.hip)
inline void opn_shape(size_t nbase, size_t n, size_t *C, size_t *n_chunks) {
    size_t c = (nbase * n) / 131072;
    if (c < 1) c = 1;
    if (c > 16) c = 16;
    if (c > nbase) c = nbase;
    *C = c;
    *n_chunks = (nbase + c - 1) / c;
}
// number of blocks of a checked segment table (seg_off[0] == 0, non-decreasing); with `out` they are written as well
inline size_t opn_blocks(const uint64_t *seg_off, size_t k, OpnBlock *out) {
    size_t nb = 0;
    for (size_t j = 0; j < k; j++) {
        const uint64_t lo = seg_off[j], m = seg_off[j + 1] - lo;
        for (uint64_t first = 0; first < m; first += OPN_WAVE, nb++)
            if (out) out[nb] = OpnBlock{lo + first, (uint32_t)j, (uint32_t)m, (uint32_t)(m - first < OPN_WAVE ? m - first : OPN_WAVE), 0};
    }
    return nb;
}

// One (identity, chunk of bases): coeff_at(i) = coefficient i of the identity's batch polynomial f, canonical (fr_poly_coeff_in), i <= m;
// id = the identity's scalar; [c_lo, c_hi) = the lane's bases, c_hi <= nbase.  The affine partial sum goes to `out` through store(out,
// point).  whole: the lane's chunk is the whole table, so it masks a row that is not ok itself; otherwise the row is masked after the
// chunks have been added, by whoever reads *ok.  ok (may be null) is written by the lane with c_lo == 0 only.
template <class F, class CoeffAt, class StoreAff>
GPBC_INLINE void fb_openings_lane(const int32_t *table, const uint8_t *base_inf, const CoeffAt &coeff_at, uint32_t m, const uint8_t *id, uint32_t c_lo, uint32_t c_hi, bool whole,
                                  uint8_t *out, uint8_t *ok, const StoreAff &store) {
    JacP<F> acc;
    jac_set_inf(acc);
    if (c_lo < m) {
        const Fr point = fr_poly_point(id);
        const bool decide = c_lo == 0;
        const uint32_t hi = c_hi < m ? c_hi : m;
        Fr carry = fr_zero(), at_id = fr_zero();                                        // at_id: q(id) over the coefficients so far
        for (uint32_t c = m; c-- > hi;) {                                               // the steps above the chunk: no group work
            carry = fr_poly_horner_step(carry, coeff_at(c + 1), point);
            if (decide) at_id = fr_poly_horner_step(at_id, carry, point);
        }
        for (uint32_t c = hi; c-- > c_lo;) {
            carry = fr_poly_horner_step(carry, coeff_at(c + 1), point);                 // quotient coefficient c
            if (decide) at_id = fr_poly_horner_step(at_id, carry, point);
            if (base_inf[c]) continue;
            uint32_t k[8];
            fr_words(k, carry);
            const int32_t *tb = table + (size_t)c * OPN_ENTRIES * TabLayout<F>::ENTRY_DWORDS;
            for (int w = 0; w < OPN_WINDOWS; w++) {
                const int d = (int)((k[w >> 2] >> (8 * (w & 3))) & 255u);
                if (d) {
                    AffP<F> e;
                    tab_load(tb + (size_t)(w * OPN_DIGITS + d - 1) * TabLayout<F>::ENTRY_DWORDS, 0, e);
                    jac_add_mixed(acc, acc, e);
                }
            }
        }
        if (decide) {
            const bool good = fr_limbs_zero(fr_poly_horner_step(carry, coeff_at(0), point)) && !fr_limbs_zero(at_id);
            if (ok) *ok = good ? 1 : 0;
            if (whole && !good) jac_set_inf(acc);
        }
    }
    AffP<F> a;
    jac_to_affine(a, acc);                                               // infinity: x = y = 0, stored as the all-zero encoding
    store(out, a);
}

}  // namespace gpbc
#endif
