// Indexed sums over the fixed-base window tables of csrc/gpbc_curve.hip for gfx950: out[i] = sum_t [k_(i,t)] base[index_(i,t)], one or
// a few public bases per output picked by an index row.  The encrypt and key-generation loops of the LSSS schemes and of BSW07 are of
// this shape: C_x = [lambda_x] g1^a + [-r_x] h_rho(x) (cpabe/waters11/waters11_cpabe.go:211-228), K_x = [t] h_x (:153-156),
// c3x = [r_x] g2^y_rho(x) + [omega_x] g2 (dabe/lw11_dabe.go:154-157), Cy' = [q_y(0)] H1(att(y)) (cpabe/bsw07/bsw07_cpabe.go Encrypt).
// The lane function and the lane-to-output mapping live here so that the kernels (k_g1_fb_indexed / k_g2_fb_indexed) and the host
// harness (tools/bounds_check.cpp: hc_fb_indexed) run the same code; neither uses blockIdx.
//
// A term is what fb_msm_lane does for one base: the scalar as it is through 32 windows of 8 bits, per non-zero digit one table row
// ([d 2^(8w)] base, affine) and one mixed addition, no doublings.  jac_add_mixed is the complete law (a doubling inside the chain, a
// cancellation to infinity and the restart after it are its exceptional branches), so terms on equal bases, on one base with k and
// r - k, and any scalar up to 2^256 - 1 come out as the group says.
#ifndef GPBC_FBINDEX29_HIP_HPP
#define GPBC_FBINDEX29_HIP_HPP
#include "curve29.hip.hpp"

namespace gpbc {

constexpr int FBI_WINDOWS = 32, FBI_DIGITS = 255, FBI_ENTRIES = FBI_WINDOWS * FBI_DIGITS;     // the table geometry of gpbc_curve.hip (FB_*)
constexpr uint32_t FBI_NONE = 0xffffffffu;                                                     // GPBC_INDEX_NONE
constexpr size_t FBI_MAX_TERMS = 16;
constexpr int FBI_WAVE = 64;

// Which output a lane owns.  Natural order: output = global lane.  With periodic index rows (P = n_index_rows < n) that order puts 64
// different index rows, so up to 64 different tables of 1-2 MB, into one wave.  The grouped order gives a workgroup 64 outputs of ONE
// index row, i = q P + rho, and numbers the workgroups index-row-major (all of row 0, then all of row 1, ...): a wave's gathers stay
// inside the tables its one row names, and the workgroups in flight at a time touch a few rows' tables.  Q = ceil(n / P) outputs per
// row at most, bpr = ceil(Q / 64) workgroups per row; taken when a row fills at least one wave (Q >= group_min), since below that the
// grouped order leaves lanes idle.
struct FbIndexMap { size_t n, P, bpr; bool grouped; };
inline FbIndexMap fb_index_map(size_t n, size_t n_index_rows, size_t group_min) {
    FbIndexMap m;
    m.n = n; m.P = n_index_rows;
    const size_t Q = (n + n_index_rows - 1) / n_index_rows;
    m.grouped = n_index_rows < n && Q >= group_min;
    m.bpr = (Q + FBI_WAVE - 1) / FBI_WAVE;
    return m;
}
GPBC_INLINE size_t fb_index_grid(const FbIndexMap &m) { return m.grouped ? m.P * m.bpr : (m.n + FBI_WAVE - 1) / FBI_WAVE; }
// the lane's output, or m.n (no output)
GPBC_INLINE size_t fb_index_output(const FbIndexMap &m, size_t block, uint32_t lane) {
    if (!m.grouped) { const size_t i = block * FBI_WAVE + lane; return i < m.n ? i : m.n; }
    const size_t rho = block / m.bpr, q = (block % m.bpr) * FBI_WAVE + lane;
    if (q > (m.n - 1 - rho) / m.P) return m.n;                      // rho < P <= n; no overflow in q P + rho below n
    return q * m.P + rho;
}

// One output: idx = its index row (terms entries), scalars = its terms scalars, out = its point, ok = its flag or null.  Every index is
// checked against nbase BEFORE anything is read through it; an index >= nbase other than FBI_NONE zeroes the row and clears the flag.
// StoreAff(out, affine point) writes the ABI's point; load_k(k, p) reads a scalar's eight words.
template <class F, class LoadScalar, class StoreAff>
GPBC_INLINE void fb_indexed_lane(const int32_t *table, const uint8_t *base_inf, size_t nbase, const uint32_t *idx, uint32_t terms, const uint8_t *scalars, uint8_t *out,
                                 uint8_t *ok, const LoadScalar &load_k, const StoreAff &store) {
    bool good = true;
    for (uint32_t t = 0; t < terms; t++) good = good && (idx[t] == FBI_NONE || (size_t)idx[t] < nbase);
    if (ok) *ok = good ? 1 : 0;
    JacP<F> acc;
    jac_set_inf(acc);
    for (uint32_t t = 0; good && t < terms; t++) {
        const uint32_t j = idx[t];
        if (j == FBI_NONE || base_inf[j]) continue;
        uint32_t k[8];
        load_k(k, scalars + 32 * (size_t)t);
        const int32_t *tb = table + (size_t)j * FBI_ENTRIES * TabLayout<F>::ENTRY_DWORDS;
        for (int w = 0; w < FBI_WINDOWS; w++) {
            const int d = (int)((k[w >> 2] >> (8 * (w & 3))) & 255u);
            if (d) {
                AffP<F> e;
                tab_load(tb + (size_t)(w * FBI_DIGITS + d - 1) * TabLayout<F>::ENTRY_DWORDS, 0, e);
                jac_add_mixed(acc, acc, e);
            }
        }
    }
    AffP<F> a;
    jac_to_affine(a, acc);                                           // infinity: x = y = 0, stored as the all-zero encoding
    store(out, a);
}

}  // namespace gpbc
#endif
