// Bit-selected sums over a fixed set in G1 / G2: out = O + sum_{i : bit i of the mask} B_i for nbits points B_0 .. B_{nbits-1}, an
// optional offset point O and one bit string per item (the Waters hash U' + sum_{Id[i]=1} U_i of ibe/waters05_ibe/waters05_ibe.go:172-179,
// 226-233; the keys of the members a participation bitmap names, gka/agka09/asbb.go:193-220).  The fixed-base tables of gpbc_curve.hip
// turned round: 8-bit windows over the BIT STRING instead of over a scalar.
//
// Table.  W = ceil(nbits / 8) windows of 256 entries; entry (w, v) at row w * 256 + v is the subset sum
//     sum_{t : (v >> (7 - t)) & 1, 8w + t < nbits} B_{8w+t}      (+ O for w = 0)
// — bit 7 - t of mask byte w selects B_{8w+t}, the reference's order (NewWaters05IBEIdentity, most significant bit first) and
// numpy.packbits' default; positions >= nbits of the last byte select nothing because the table ignores them, so a lane never masks a
// byte.  With O folded into window 0 no item adds O itself.  Rows are affine points in the internal limb form and the 128-byte-aligned
// row layout of curve29.hip.hpp (tab_store / tab_load: 128 B per G1 row, 256 B per G2 row), and every row has a one-byte flag: 1 = the
// point at infinity (v = 0 without an offset, every selected base at infinity, bases that cancel, an offset that cancels them) — the
// row then holds zeros and is not added.  Build: one lane per entry, at most nine jac_add_mixed and one jac_to_affine.
//
// Sum.  One lane per (item, chunk of C windows) walks its windows with one jac_add_mixed per window whose entry is not flagged — no
// doublings; jac_add_mixed turns "entry equals the accumulator" into a doubling and "entry is minus the accumulator" into infinity —
// and converts to affine once.  The next row is requested one step ahead, the mask byte two steps ahead.  EVERY lane walks C windows:
// a window past W (the last chunk when C does not divide W) is walked with the addition switched off, like a flagged entry, so the
// lanes of a wavefront never run different trip counts (csrc/gmsm29.hip.hpp records wrong G2 sums on gfx950 where they did).
//
// Chunks (subset_shape): a call whose n alone fills the chip takes C = W, one lane per item, and writes the results itself; a smaller
// one cuts the windows into up to W / SUBSET_CHUNK_MIN chunks, writes the partial sums chunk-major (partial[c * n + m]) and ONE launch
// of the strided point-sum kernel adds the chunks of every item, as gpbc_fixed_base_msm_dev does.  A chunk costs a conversion to
// affine — an inversion, about as many products as 30 additions — and an addition in the fold, so none is shorter than 32 windows.
// The same file is the host interval harness's (tools/bounds_check.cpp, hc_subset_sum): one entry function, one lane function, one shape.
#ifndef GPBC_SUBSET29_HIP_HPP
#define GPBC_SUBSET29_HIP_HPP
#include "curve29.hip.hpp"

namespace gpbc {

constexpr size_t SUBSET_MAX_BITS = 16384;                                    // 2 048 windows: 524 288 rows, 64 MiB (G1) / 128 MiB (G2) + 512 KiB of flags
constexpr size_t SUBSET_FILL = 131072;                                       // lanes that fill the chip: 256 CUs x 4 SIMDs x 2 waves x 64 lanes
constexpr size_t SUBSET_CHUNK_MIN = 32;                                      // windows per chunk at least (see above)

GPBC_INLINE size_t subset_windows(size_t nbits) { return (nbits + 7) / 8; }
GPBC_INLINE size_t subset_entries(size_t nbits) { return subset_windows(nbits) * 256; }
// C windows per lane, n_chunks = ceil(W / C) lanes per item; from W and n alone
GPBC_INLINE void subset_shape(size_t W, size_t n, size_t &C, size_t &n_chunks) {
    size_t want = n ? (SUBSET_FILL + n - 1) / n : 1;
    const size_t most = W / SUBSET_CHUNK_MIN;
    if (want > most) want = most;
    if (want < 1) want = 1;
    C = (W + want - 1) / want;
    n_chunks = (W + C - 1) / C;
}

// entry (w, v) of the table as an affine point (a.inf: the point at infinity, a.x = a.y = 0); base(i) = B_i
template <class F, class Base> GPBC_INLINE void subset_entry(AffP<F> &a, Base base, size_t nbits, const AffP<F> *offset, size_t w, int v) {
    JacP<F> r;
    jac_set_inf(r);
    if (w == 0 && offset) jac_add_mixed(r, r, *offset);
    for (int t = 0; t < 8; t++) {
        const size_t i = 8 * w + (size_t)t;
        if (i < nbits && ((v >> (7 - t)) & 1)) jac_add_mixed(r, r, base(i));
    }
    jac_to_affine(a, r);
}
template <class F> GPBC_INLINE void subset_entry_store(int32_t *table, uint8_t *flags, size_t e, const AffP<F> &a) {
    tab_store(table + e * (size_t)TabLayout<F>::ENTRY_DWORDS, 0, a);
    flags[e] = a.inf ? 1 : 0;
}

// the sum of windows [w0, w0 + C) of one item: mask = the item's W bytes
template <class F> GPBC_INLINE JacP<F> subset_lane(const int32_t *table, const uint8_t *flags, const uint8_t *mask, size_t W, size_t w0, size_t C) {
    constexpr size_t ED = (size_t)TabLayout<F>::ENTRY_DWORDS;
    JacP<F> acc;
    jac_set_inf(acc);
    // a window past W reads the row of (W - 1, 0) — inside the table — and is never added
    auto byte_at = [&](size_t j) { const size_t w = w0 + (j < C ? j : C - 1); return w < W ? (uint32_t)mask[w] : 0u; };
    auto row_of = [&](size_t j, uint32_t b) { const size_t w = w0 + j; return (w < W ? w : W - 1) * 256 + (w < W ? b : 0u); };
    size_t e = row_of(0, byte_at(0));
    AffP<F> t;
    tab_load(table + e * ED, 0, t);
    bool skip = w0 >= W || flags[e] != 0;
    uint32_t b1 = byte_at(1);
#pragma unroll 1
    for (size_t j = 0; j < C; j++) {
        const size_t jn = j + 1 < C ? j + 1 : j;
        const uint32_t b2 = byte_at(j + 2);
        const size_t en = row_of(jn, b1);
        AffP<F> nx;
        tab_load(table + en * ED, 0, nx);
        const bool nskip = w0 + jn >= W || flags[en] != 0;
        if (!skip) jac_add_mixed(acc, acc, t);                              // equal or opposite to the accumulator: doubling / infinity, handled there
        t = nx; skip = nskip; b1 = b2;
    }
    return acc;
}

}  // namespace gpbc
#endif
