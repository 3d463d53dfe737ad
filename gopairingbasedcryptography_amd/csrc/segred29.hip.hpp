// Segmented reductions, the part that does not depend on what is reduced: out[s] = the reduction of x[seg_off[s] .. seg_off[s+1])
// (optionally with one 256-bit scalar k per element, or one list of nk for every segment).  One level = every segment cut into J
// pieces, one worker (a lane, a lane pair) per piece; J > 1 leaves n_seg x J piece values, which the next level folds as uniform
// segments of J values in plain mode (no k), and so on until J = 1 writes `out`.  This file holds the cut, the kernel argument, the
// level walk and the workspace plan; the segmented GT multi-exponentiation (csrc/gtmexp29.hip.hpp) and the segmented G1 / G2
// multi-scalar multiplication (csrc/gmsm29.hip.hpp) each add a shape and their lane functions.  The kernels, the host driver
// (segred_dev, csrc/gpbc_core.hip) and the host interval harness (tools/bounds_check.cpp) run this one plan.
#ifndef GPBC_SEGRED29_HIP_HPP
#define GPBC_SEGRED29_HIP_HPP
#include "fe29.hip.hpp"

namespace gpbc {

struct SegRedShape {
    size_t fill;                          // workers that fill the chip; also the most pieces of one launch
    size_t group;                         // elements with scalars that share one chain of squarings / doublings
    size_t plain_min;                     // a piece in plain mode has at least this many elements on average
};

// Pieces per segment, from the sizes alone (the segment table may live in device memory): enough pieces to fill the chip, but none
// shorter on average than one group (with scalars) or plain_min elements (plain mode).  1 = no cut: the worker of a segment writes
// the result itself.  n_seg x J <= fill + n_seg whatever the segment lengths are.
GPBC_INLINE size_t segred_pieces(const SegRedShape &sh, size_t n, size_t n_seg, bool has_k) {
    if (!n_seg) return 1;
    const size_t by_len = (n / n_seg) / (has_k ? sh.group : sh.plain_min);
    const size_t by_fill = (sh.fill + n_seg - 1) / n_seg;
    const size_t j = by_len < by_fill ? by_len : by_fill;
    return j ? j : 1;
}
// Segment s as [lo, hi): from the table with every offset clamped to n (a malformed table shortens segments, it never reaches outside
// x), or, without a table (the folds), uniform segments of m; with a shared scalar list (nk_shared != 0) a segment ends after
// nk_shared elements, so the list is never overrun.
GPBC_INLINE void segred_segment_range(const uint64_t *seg_off, size_t m, size_t n, size_t s, size_t nk_shared, size_t &lo, size_t &hi) {
    if (seg_off) {
        const uint64_t o0 = seg_off[s], o1 = seg_off[s + 1];
        lo = o0 < n ? (size_t)o0 : n;
        hi = o1 < n ? (size_t)o1 : n;
        if (hi < lo) hi = lo;
    } else { lo = s * m; hi = lo + m; }
    if (nk_shared && hi - lo > nk_shared) hi = lo + nk_shared;
}
// Elements [a, b) of piece j of J of the segment [lo, hi): the J pieces tile the segment, their lengths differ by at most one.
GPBC_INLINE void segred_piece_range(size_t lo, size_t hi, size_t j, size_t J, size_t &a, size_t &b) {
    const size_t len = hi - lo;
    a = lo + (size_t)((uint64_t)len * j / J);                               // len < 2^46, J <= 2^17 + 1: no overflow
    b = lo + (size_t)((uint64_t)len * (j + 1) / J);
}

// What a worker works on: piece P = piece0 + (its index in the launch) is piece P % J of segment P / J.
struct SegRedArgs {
    const uint8_t *x, *k;                 // k: null = plain mode
    size_t nk;
    int k_shared;                         // 1: k holds one list of nk scalars for every segment
    const uint64_t *seg_off;              // null: uniform segments of m elements
    size_t m, n, n_seg, J, piece0, n_pieces;
    uint8_t *out;                         // piece results, one element each, at index piece0 + index
};
GPBC_INLINE SegRedArgs segred_args(const void *x, const void *k, size_t nk, const uint64_t *seg_off, size_t n, size_t n_seg) {
    return SegRedArgs{(const uint8_t *)x, (const uint8_t *)k, nk, k && nk != n, seg_off, 0, n, n_seg, 0, 0, 0, nullptr};
}
GPBC_INLINE bool segred_piece(const SegRedArgs &g, size_t index, size_t &lo, size_t &a, size_t &b, size_t &P) {
    if (index >= g.n_pieces) return false;
    P = g.piece0 + index;
    size_t hi;
    segred_segment_range(g.seg_off, g.m, g.n, P / g.J, g.k && g.k_shared ? g.nk : 0, lo, hi);
    segred_piece_range(lo, hi, P % g.J, g.J, a, b);
    return true;
}

// The levels of a call from its sizes alone: level(index, J, pieces) until it fails or J = 1.
template <class Level> inline int segred_levels(const SegRedShape &sh, size_t n, size_t n_seg, bool has_k, Level level) {
    for (int lv = 0;; lv++) {
        const size_t J = segred_pieces(sh, n, n_seg, has_k), pieces = n_seg * J;
        const int rc = level(lv, J, pieces);
        if (rc || J == 1) return rc;
        n = pieces; has_k = false;
    }
}
// The same walk with the arguments: level(g, pieces) gets J and out set (the value buffer of the level's parity, or `out` at J = 1)
// and runs pieces [0, pieces) — it sets piece0 / n_pieces in its copy; what it leaves is then the next level's input, n_seg uniform
// segments of J values in plain mode.
template <class Level> inline int segred_walk(const SegRedShape &sh, SegRedArgs g, uint8_t *const *val, void *out, Level level) {
    return segred_levels(sh, g.n, g.n_seg, g.k != nullptr, [&](int lv, size_t J, size_t pieces) {
        g.J = J;
        g.out = J > 1 ? val[lv & 1] : (uint8_t *)out;
        const int rc = level(g, pieces);
        g = SegRedArgs{g.out, nullptr, 0, 0, nullptr, J, pieces, g.n_seg, 0, 0, 0, nullptr};
        return rc;
    });
}

// workspace layout: [tables of one launch | piece values of the even levels | piece values of the odd levels], every part a whole
// number of 256-byte granules
struct SegRedPlan {
    size_t tab_bytes, val_bytes[2];
    size_t bytes() const { return tab_bytes + val_bytes[0] + val_bytes[1]; }
};
inline size_t segred_padded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
inline SegRedPlan segred_plan(const SegRedShape &sh, size_t elem_bytes, size_t tab_bytes_per_piece, size_t n, size_t n_seg, bool has_k) {
    SegRedPlan p{0, {0, 0}};
    if (!n_seg) return p;
    segred_levels(sh, n, n_seg, has_k, [&](int lv, size_t J, size_t pieces) {
        if (lv == 0 && has_k) p.tab_bytes = segred_padded((pieces < sh.fill ? pieces : sh.fill) * tab_bytes_per_piece);
        const size_t bytes = J > 1 ? segred_padded(pieces * elem_bytes) : 0;
        if (p.val_bytes[lv & 1] < bytes) p.val_bytes[lv & 1] = bytes;
        return 0;
    });
    return p;
}

}  // namespace gpbc
#endif
