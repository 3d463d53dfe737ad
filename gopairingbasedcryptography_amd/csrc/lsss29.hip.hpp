// LSSS share generation in Fr for gfx950: lambda_x = M_x . v for every row x of a share-generating matrix and k vectors v = (s, v_2, ..)
// per call (LewkoWatersLsssMatrix.ComputeVector of the reference, access/lsss/lewko_waters_lsss_matrix.go:131-141, as cpabe/waters11
// Encrypt and dabe/lw11 Encrypt call it once per ciphertext).  Built on fr29.hip.hpp; the kernel (k_fr_lsss_shares in csrc/gpbc_fr.hip)
// and the host harness (tools/bounds_check.cpp: hc_fr_lsss_shares) differ only in where a staged matrix waits.
//
// One lane per output share (j, x).  Nothing is converted on the way in: a matrix entry and a vector element are their 32 bytes cut into
// nine limbs (fr_load_raw: any value below 2^256 < 5.3 r, limbs 0..7 in [0, 2^29), limb 8 below 2^24), and two of their products share one
// reduction, t = (m_c v_c + m_(c+1) v_(c+1)) / 2^261 (fr_mul2_inline; an odd last column is one product):
//   columns of the product   2 x 9 x 2^29 x 2^29 < 2^62.2, plus the reduction's 9 x 2^58 and the carry: below 2^63
//   t                        in (-eps r, (1 + eps) r) with eps = 2 x 5.3^2 x r / 2^261 < 0.34; limbs 0..7 in [0, 2^29), limb 8 below 2^23
// The sum of the t is carry-free (fr_add) and normalised (fr_norm: every limb keeps its low 29 bits and takes its neighbour's carry)
// after every FR_LSSS_SHARES_NORM = 2 additions, so a limb of the accumulator stays below 2^29 + 4 + 2 x 2^29 < 2^31 and its top limb
// below 32 x 1.34 x r / 2^232 < 2^28; the value stays below 32 x 1.34 r < 43 r for the 64 columns the entry allows.  The last step
// multiplies the (normalised) sum by 2^522 mod r, which takes the factor 2^-261 of the products back and reduces in one: columns below
// 9 x (2^29 + 4) x 2^29 < 2^62, result in (-0.26 r, 1.26 r).  Only that is made canonical (fr_canonical<1, 2>: (-r, 2 r)).
// All of it is asserted under -DGPBC_BOUNDS for the interval classes, not for the values of a run.
#ifndef GPBC_LSSS29_HIP_HPP
#define GPBC_LSSS29_HIP_HPP
#include "fr29.hip.hpp"

namespace gpbc {

constexpr int FR_LSSS_SHARES_WAVE = 64, FR_LSSS_SHARES_NORM = 2;
// elem_at(c): entry c of the lane's matrix row as it was staged or as it lies in memory; vec: the item's `cols` scalars
template <class ElemAt> GPBC_INLINE void fr_lsss_shares_lane(const ElemAt &elem_at, uint32_t cols, const uint8_t *vec, uint8_t *out) {
    Fr acc = fr_zero();
    uint32_t pending = 0;
    for (uint32_t c = 0; c + 1 < cols; c += 2) {
        acc = fr_add(acc, fr_mul2_inline(elem_at(c), fr_load_raw(vec + 32 * (size_t)c), elem_at(c + 1), fr_load_raw(vec + 32 * (size_t)(c + 1))));
        if (++pending == (uint32_t)FR_LSSS_SHARES_NORM) { acc = fr_norm(acc); pending = 0; }
    }
    if (cols & 1u) acc = fr_add(acc, fr_mul(elem_at(cols - 1), fr_load_raw(vec + 32 * (size_t)(cols - 1))));
    fr_store_canonical(out, fr_canonical<1, 2>(fr_to_internal(fr_norm(acc))));
}

// The launch: one wave per workgroup.  A workgroup owns rg consecutive rows of the matrix (a "row group") for ipb = 64 / rg items:
// lane = (local item) x rg + (row in the group), so the rg shares of an item are neighbouring lanes (one contiguous store per item) and
// the lanes of an item read one vector address (a broadcast).  rg = min(rows, 64), and with ONE matrix for all items also at most
// FR_SHARES_CAP / cols (>= 4): the workgroup stages its row group once in LDS, unconverted, row xr at word xr x pitch, entry c at
// + c x NL, pitch odd (the lanes of an item read different banks).  The block is 9.3 KB, sixteen workgroups per CU: 16 x 15 fits whole,
// 64 x 64 takes sixteen row groups of 4 rows.  With a matrix per item there is nothing to share: a lane reads its own row from memory.
constexpr int FR_SHARES_CAP = 256;
struct LsssSharesGeom { uint32_t rows, cols, rg, nrg, ipb, pitch; };
struct LsssSharesLane { size_t item; uint32_t x, xr; bool active; };
inline LsssSharesGeom fr_lsss_shares_geometry(size_t rows, size_t cols, bool shared_matrix) {
    LsssSharesGeom g;
    g.rows = (uint32_t)rows; g.cols = (uint32_t)cols;
    g.rg = g.rows < (uint32_t)FR_LSSS_SHARES_WAVE ? g.rows : (uint32_t)FR_LSSS_SHARES_WAVE;
    const uint32_t fit = (uint32_t)FR_SHARES_CAP / g.cols;       // >= 4: cols <= 64
    if (shared_matrix && g.rg > fit) g.rg = fit;
    g.nrg = (g.rows + g.rg - 1) / g.rg;
    g.ipb = (uint32_t)FR_LSSS_SHARES_WAVE / g.rg;
    g.pitch = (g.cols * NL) | 1u;
    return g;
}
GPBC_INLINE size_t fr_lsss_shares_grid(const LsssSharesGeom &g, size_t k) { return (k + g.ipb - 1) / g.ipb * g.nrg; }
GPBC_INLINE uint32_t fr_lsss_shares_group_rows(const LsssSharesGeom &g, uint32_t block) {
    const uint32_t x0 = (block % g.nrg) * g.rg, left = g.rows - x0;
    return left < g.rg ? left : g.rg;
}
// a lane's share of the staging of the ONE matrix: put(word offset, raw entry)
template <class Put> GPBC_INLINE void fr_lsss_shares_stage(const LsssSharesGeom &g, uint32_t block, uint32_t lane, const uint8_t *matrix, const Put &put) {
    const uint32_t x0 = (block % g.nrg) * g.rg, total = fr_lsss_shares_group_rows(g, block) * g.cols;
    for (uint32_t idx = lane; idx < total; idx += FR_LSSS_SHARES_WAVE) {
        const uint32_t xr = idx / g.cols, c = idx % g.cols;
        put(xr * g.pitch + c * NL, fr_load_raw(matrix + 32 * ((size_t)(x0 + xr) * g.cols + c)));
    }
}
GPBC_INLINE LsssSharesLane fr_lsss_shares_map(const LsssSharesGeom &g, uint32_t block, uint32_t lane, size_t k) {
    LsssSharesLane l;
    const uint32_t li = lane / g.rg;
    l.xr = lane % g.rg;
    l.x = (block % g.nrg) * g.rg + l.xr;
    l.item = (size_t)(block / g.nrg) * g.ipb + li;
    l.active = li < g.ipb && l.item < k && l.x < g.rows;
    return l;
}

}  // namespace gpbc
#endif
