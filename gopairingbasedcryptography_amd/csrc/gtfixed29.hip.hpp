// Fixed-base exponentiation in GT for gfx950: window tables of public Fp12 elements kept in HBM, and products of a few of their powers
// per output, out[i] = prod_t base[index_(i,t)] ^ k_(i,t).  Every Encrypt of the reference raises one public GT element to a fresh
// scalar: e(g1, g2)^s (ibe/bb04_sibe/bb04_sibe.go:195-200), e(g1^alpha, g2)^t (ibe/bb04_ibe/bb04_ibe.go:181-189,
// ibe/waters05_ibe/waters05_ibe.go:214), e(g,g)^s, e(g,h1)^-s and e(g,h2)^s e(g,h3)^(s beta) (ibe/gentry06_ibe/gentry06_ibe.go:192-245).
// The lane functions live here so that the kernels (csrc/gpbc_gtfixed.hip: k_gt_fb_build, k_gt_fb_indexed) and the host harness
// (tools/bounds_check.cpp: hc_gt_fb_build, hc_gt_fb_indexed) run the same code; neither uses blockIdx.
//
// Geometry: that of the G1 / G2 tables (fbindex29.hip.hpp), 32 windows of 8 bits, with the digit 0 stored as well: entry (j, w, d) is
// base_j ^ (d 2^(8w)), d = 0 .. 255, and d = 0 is one — a term then multiplies once per window whatever the digit, and no lane pair
// waits for another's branch (what f12p_exp256 does with its sixteen entries).  One Fp12 value per LANE PAIR (tower29_pair.hip.hpp):
// an entry is two half-rows of GT_EXP_ROW_DWORDS int32, the even lane's C0 and then the odd lane's C1, each written by f6_row_store
// after f6_norm and read by f6_row_load: 512 bytes per entry, 32 x 256 x 512 B = 4 MiB per base.
//
// Bases are ANY Fp12 element, as for gnark's Exp: the squarings are the generic ones, and a zero base gives zero for k > 0 and one for
// k = 0 (its entries are zero for d > 0 and one for d = 0).  Scalars are used as the integers they are, below 2^256.
//
// Limb bounds: the running product is f12p_mul(output of f12p_mul, normalised table entry) up to 16 x 32 times, the shape of the
// table-building loop of f12p_exp256; f12p_mul ends in f6_reduce(f6_norm(.)), so its output is in one interval class whatever went in,
// and the class of a table entry is the one f6_row_load declares.  The host interval build (GPBC_BOUNDS) runs both lane functions.
#ifndef GPBC_GTFIXED29_HIP_HPP
#define GPBC_GTFIXED29_HIP_HPP
#include "fbindex29.hip.hpp"
#include "pairing29_pair.hip.hpp"

namespace gpbc {

constexpr int GTFB_WINDOWS = FBI_WINDOWS, GTFB_DIGITS = FBI_DIGITS + 1;                       // d = 0 .. 255: the zero digit has an entry
constexpr size_t GTFB_ENTRY_DWORDS = 2 * (size_t)GT_EXP_ROW_DWORDS;                           // C0's half-row, then C1's
constexpr size_t GTFB_WINDOW_DWORDS = (size_t)GTFB_DIGITS * GTFB_ENTRY_DWORDS;
constexpr size_t GTFB_BASE_DWORDS = (size_t)GTFB_WINDOWS * GTFB_WINDOW_DWORDS;                // 4 MiB of int32 per base
static_assert(GTFB_BASE_DWORDS * sizeof(int32_t) == (size_t)4 << 20, "32 x 256 x 512 B per base");

// One (base, window) on a lane pair: half = this lane's 192 bytes of the base (even lane C0, odd lane C1), win = the window's 256
// entries.  b^(2^(8w)) by 8 w generic squarings; the loop runs 8 w_max times for every pair and a pair keeps the value it passes at
// its own 8 w — w_max is the largest window of the wavefront (31 on the device, so the wavefront's pairs stay in step; the pair's own
// w in the host harness, where the pair is the wavefront).  Then entry d = entry (d - 1) * entry 1, each stored normalised.
template <class X> GPBC_INLINE void gt_fb_build_lane(const X &x, const uint8_t *half, int w, int w_max, int32_t *win) {
    int32_t *row = win + (x.odd ? GT_EXP_ROW_DWORDS : 0);
    f6_row_store(row, f6_norm(f12p_one(x)));
    F6 cur = f6_load(half), e1 = cur;
#pragma unroll 1
    for (int s = 1; s <= 8 * w_max; s++) {
        cur = f6_reduce(f12p_sqr(x, cur));
        e1 = f6_sel(s == 8 * w, cur, e1);
    }
    e1 = f6_norm(e1);
    f6_row_store(row + GTFB_ENTRY_DWORDS, e1);
    cur = e1;
#pragma unroll 1
    for (int d = 2; d < GTFB_DIGITS; d++) {
        cur = f12p_mul(x, cur, e1);
        f6_row_store(row + (size_t)d * GTFB_ENTRY_DWORDS, f6_norm(cur));
    }
}

// One output on a lane pair: idx = its index row (terms entries), scalars = its terms scalars, out_half = this lane's 192 bytes of the
// output, ok = its flag or null (the even lane writes it).  Every index is checked against nbase BEFORE an address is formed from it;
// an index >= nbase other than FBI_NONE zeroes the row, clears the flag and the pair leaves together.  A term that is FBI_NONE is
// skipped when the whole wavefront has none there (one vote, outside any per-pair branch); beside a neighbour that has one, the pair
// multiplies by the entries d = 0 of base 0, which are one.  Per term and window: one f6_row_load of this lane's half-row and one
// f12p_mul into the running product; no squarings.  load_k(k, p) reads a scalar's eight words.
template <class X, class LoadScalar>
GPBC_INLINE void gt_fb_indexed_lane(const X &x, const int32_t *table, size_t nbase, const uint32_t *idx, uint32_t terms, const uint8_t *scalars, uint8_t *out_half,
                                    uint8_t *ok, const LoadScalar &load_k) {
    bool good = true;
    for (uint32_t t = 0; t < terms; t++) good = good && (idx[t] == FBI_NONE || (size_t)idx[t] < nbase);
    if (ok && !x.odd) *ok = good ? 1 : 0;
    if (!good) {
        uint32_t *z = reinterpret_cast<uint32_t *>(out_half);
        for (int i = 0; i < 48; i++) z[i] = 0;
        return;
    }
    const int32_t *mine = table + (x.odd ? GT_EXP_ROW_DWORDS : 0);
    F6 r = f12p_one(x);
#pragma unroll 1
    for (uint32_t t = 0; t < terms; t++) {
        const uint32_t j = idx[t];
        const bool none = j == FBI_NONE;
        if (x.all(none)) continue;
        uint32_t k[8];
        load_k(k, scalars + 32 * (size_t)t);
        const int32_t *tb = mine + (none ? (size_t)0 : (size_t)j) * GTFB_BASE_DWORDS;
#pragma unroll 1
        for (int w = 0; w < GTFB_WINDOWS; w++) {
            const uint32_t d = none ? 0u : k[0] & 255u;
#pragma unroll
            for (int i = 0; i < 7; i++) k[i] = (k[i] >> 8) | (k[i + 1] << 24);     // the next digit moves down: no register array indexed by w
            k[7] >>= 8;
            r = f12p_mul(x, r, f6_row_load(tb + (size_t)w * GTFB_WINDOW_DWORDS + (size_t)d * GTFB_ENTRY_DWORDS));
        }
    }
    f6_store(out_half, r);
}

}  // namespace gpbc
#endif
