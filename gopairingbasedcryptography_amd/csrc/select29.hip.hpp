// The common attributes of a list and a set in Fr for gfx950: utils.FindCommonAttributes of the reference (utils/find_common_attributes.go:7-35)
// for k items at once, with the positions sw05.select_common adds — what SW05 Decrypt (fibe/sw05_fibe_common.go:284-333) decides per
// ciphertext before it takes a Lagrange coefficient.  Per item: a list of `a` values (the ciphertext's attributes) and a set of `m` values
// (the key's, one set for all items or one per item), any integers below 2^256, compared as field elements (modulo r).  The definition:
//   walk the list in order; KEEP an element iff the set holds it and no earlier list element equal to it was kept; stop after d kept
//   elements; a kept element's set position is its FIRST occurrence in the set; with fewer than d kept the item is not decryptable:
//   ok = 0 and all-zero rows.
// Built on fr29.hip.hpp's load and canonical form; the kernel (k_fr_find_common in csrc/gpbc_fr.hip) and the host harness
// (tools/bounds_check.cpp) differ only in where the staged words wait.
//
// One wave per workgroup.  A lane owns one list element at a time: lpi = min(a, 64) lanes per item, ipb = 64 / lpi items per workgroup
// (fewer when sets of their own would not fit), a > 64 walks the list in chunks of 64.  Four phases, a barrier between them, every value that
// crosses lanes waits in LDS:
//   STAGE  the set(s) of the workgroup, canonical, eight words per element (a shared set once; lanes of one item read one address);
//   MATCH  a lane makes its element canonical and scans the set from the front: the first equal element's position, or NONE, is its pos word;
//   MARK   two matched elements are equal modulo r exactly when their first set positions are, so a lane is a repeat iff an earlier pos
//          word equals its own: its keep word is 1 iff it matched and is no repeat — 32-bit compares, no field element is touched again;
//   PICK   a lane counts the keep words before its own (its rank) and all of them (ok = at least d); a kept element of rank < d writes
//          slot `rank` of the item's three rows, the value copied from the set's LDS copy (canonical, and equal to the element).
#ifndef GPBC_SELECT29_HIP_HPP
#define GPBC_SELECT29_HIP_HPP
#include "fr29.hip.hpp"

namespace gpbc {

constexpr int FR_SELECT_WAVE = 64, FR_SELECT_MAX = FR_POLY_MAX_B, FR_SELECT_EW = 8;
constexpr uint32_t FR_SELECT_NONE = 0xffffffffu;
// LDS words: cap x 8 of set elements (+ a wave of slack for the odd pitch of per-item sets), then P pos words and P keep words.
// Small: 256 staged elements and P = 64 (8.8 KB); large: 1024 and P = 1024 (40.3 KB), taken by a > 64 or more staged elements.
constexpr int FR_SELECT_SMALL_SET = 256, FR_SELECT_LARGE_SET = FR_SELECT_MAX;
GPBC_INLINE constexpr int fr_select_words(bool large) {
    return (large ? FR_SELECT_LARGE_SET : FR_SELECT_SMALL_SET) * FR_SELECT_EW + FR_SELECT_WAVE + 2 * (large ? FR_SELECT_MAX : FR_SELECT_WAVE);
}
constexpr int FR_SELECT_WORDS_SMALL = fr_select_words(false), FR_SELECT_WORDS_LARGE = fr_select_words(true);
struct SelectGeom { uint32_t m, a, d, lpi, ipb, chunks, pitch, pos0, keep0, large, shared; };
// where the rows go: item j's slot s at set_pos + j x pos_step + 4 s, list_pos likewise, common + j x common_step + 32 s (bytes); ok + j
struct SelectOut { uint8_t *set_pos, *list_pos, *common, *ok; size_t pos_step, common_step; };

inline SelectGeom fr_select_geometry(size_t m, size_t a, size_t d, bool shared) {
    SelectGeom g;
    g.m = (uint32_t)m; g.a = (uint32_t)a; g.d = (uint32_t)d; g.shared = shared ? 1u : 0u;
    g.lpi = a < (size_t)FR_SELECT_WAVE ? (uint32_t)a : (uint32_t)FR_SELECT_WAVE;
    g.chunks = (uint32_t)((a + FR_SELECT_WAVE - 1) / FR_SELECT_WAVE);
    g.ipb = (uint32_t)FR_SELECT_WAVE / g.lpi;                                     // a > 64: 1
    if (!shared) {
        const uint32_t fit = (uint32_t)((size_t)FR_SELECT_LARGE_SET / m);        // >= 1: m <= 1024
        if (g.ipb > fit) g.ipb = fit;
    }
    g.pitch = shared ? 0u : g.m * FR_SELECT_EW + 1u;                             // odd: the sets of a wave's items start in different banks
    g.large = (shared ? m : (size_t)g.ipb * m) > (size_t)FR_SELECT_SMALL_SET || a > (size_t)FR_SELECT_WAVE;
    g.pos0 = (uint32_t)((g.large ? FR_SELECT_LARGE_SET : FR_SELECT_SMALL_SET) * FR_SELECT_EW + FR_SELECT_WAVE);
    g.keep0 = g.pos0 + (uint32_t)(g.large ? FR_SELECT_MAX : FR_SELECT_WAVE);
    return g;
}
GPBC_INLINE size_t fr_select_grid(const SelectGeom &g, size_t k) { return (k + g.ipb - 1) / g.ipb; }
GPBC_INLINE uint32_t fr_select_items(const SelectGeom &g, uint32_t block, size_t k) {
    const size_t left = k - (size_t)block * g.ipb;
    return left < g.ipb ? (uint32_t)left : g.ipb;
}
// the eight words of a value of the scalar format, canonical
GPBC_INLINE void fr_select_in(uint32_t w[FR_SELECT_EW], const uint8_t *p) { fr_words(w, fr_lagrange_in(p)); }
// a lane's item and first element: li the item's number in the workgroup, le the element (of every chunk: le + 64 c), base / words the
// item's set and pos / keep words in LDS
struct SelectLane { size_t item; uint32_t li, le, base, words; bool active; };
GPBC_INLINE SelectLane fr_select_map(const SelectGeom &g, uint32_t block, uint32_t lane, size_t k) {
    SelectLane l;
    l.li = lane / g.lpi;
    l.le = lane % g.lpi;
    l.item = (size_t)block * g.ipb + l.li;
    l.base = l.li * g.pitch;
    l.words = l.li * g.a;                                                        // a <= 64: ipb x a <= 64 words; a > 64: li = 0
    l.active = l.li < fr_select_items(g, block, k);
    return l;
}
// STAGE, a lane's share: pute(word offset, the element's eight words)
template <class PutE> GPBC_INLINE void fr_select_stage(const SelectGeom &g, uint32_t block, uint32_t lane, size_t k, const uint8_t *sets, const PutE &pute) {
    const size_t item0 = (size_t)block * g.ipb, set_step = g.shared ? 0 : (size_t)g.m * 32;
    const uint32_t staged = g.shared ? 1u : fr_select_items(g, block, k);
    for (uint32_t idx = lane; idx < staged * g.m; idx += FR_SELECT_WAVE) {
        const uint32_t lr = idx / g.m, u = idx % g.m;
        uint32_t w[FR_SELECT_EW];
        fr_select_in(w, sets + (item0 + lr) * set_step + 32 * (size_t)u);
        pute(lr * g.pitch + u * FR_SELECT_EW, w);
    }
}
// MATCH: gete(element's word offset, word) reads a staged element, putw(word offset, value) writes a single word
template <class GetE, class PutW> GPBC_INLINE void fr_select_match(const SelectGeom &g, uint32_t block, uint32_t lane, size_t k, const uint8_t *lists, const GetE &gete, const PutW &putw) {
    const SelectLane l = fr_select_map(g, block, lane, k);
    if (!l.active) return;
    for (uint32_t e = l.le; e < g.a; e += FR_SELECT_WAVE) {
        uint32_t w[FR_SELECT_EW];
        fr_select_in(w, lists + (l.item * g.a + e) * 32);
        uint32_t pos = FR_SELECT_NONE;
        for (uint32_t u = 0; u < g.m; u++) {
            const uint32_t off = l.base + u * FR_SELECT_EW;
            if (gete(off, 0) != w[0]) continue;
            uint32_t diff = 0;
#pragma unroll
            for (int i = 1; i < FR_SELECT_EW; i++) diff |= gete(off, i) ^ w[i];
            if (!diff) { pos = u; break; }
        }
        putw(g.pos0 + l.words + e, pos);
    }
}
// MARK: getw(word offset) reads a single word written before the last barrier
template <class GetW, class PutW> GPBC_INLINE void fr_select_mark(const SelectGeom &g, uint32_t block, uint32_t lane, size_t k, const GetW &getw, const PutW &putw) {
    const SelectLane l = fr_select_map(g, block, lane, k);
    if (!l.active) return;
    for (uint32_t e = l.le; e < g.a; e += FR_SELECT_WAVE) {
        const uint32_t pos = getw(g.pos0 + l.words + e);
        uint32_t keep = pos != FR_SELECT_NONE ? 1u : 0u;
        for (uint32_t q = 0; keep && q < e; q++)
            if (getw(g.pos0 + l.words + q) == pos) keep = 0;
        putw(g.keep0 + l.words + e, keep);
    }
}
// PICK: emit(item, slot, set position, list position, the value's eight words) for every slot of the item's rows, done(item, ok) once
template <class GetE, class GetW, class Emit, class Done>
GPBC_INLINE void fr_select_pick(const SelectGeom &g, uint32_t block, uint32_t lane, size_t k, const GetE &gete, const GetW &getw, const Emit &emit, const Done &done) {
    const SelectLane l = fr_select_map(g, block, lane, k);
    if (!l.active) return;
    uint32_t total = 0;
    for (uint32_t q = 0; q < g.a; q++) total += getw(g.keep0 + l.words + q);
    const bool ok = total >= g.d;
    if (l.le == 0) done(l.item, ok);
    uint32_t w[FR_SELECT_EW];
    if (!ok) {
#pragma unroll
        for (int i = 0; i < FR_SELECT_EW; i++) w[i] = 0;
        for (uint32_t s = l.le; s < g.d; s += g.lpi) emit(l.item, s, 0u, 0u, w);
        return;
    }
    uint32_t rank = 0, counted = 0;                                             // rank: the keep words of [0, counted)
    for (uint32_t e = l.le; e < g.a && rank < g.d; e += FR_SELECT_WAVE) {
        for (; counted < e; counted++) rank += getw(g.keep0 + l.words + counted);
        if (rank >= g.d || !getw(g.keep0 + l.words + e)) continue;
        const uint32_t pos = getw(g.pos0 + l.words + e), off = l.base + pos * FR_SELECT_EW;
#pragma unroll
        for (int i = 0; i < FR_SELECT_EW; i++) w[i] = gete(off, i);
        emit(l.item, rank, pos, e, w);
    }
}
// the kernel's emit and done: ordinary stores into the rows SelectOut describes
GPBC_INLINE void fr_select_store(const SelectOut &o, size_t item, uint32_t slot, uint32_t set_pos, uint32_t list_pos, const uint32_t w[FR_SELECT_EW]) {
    reinterpret_cast<uint32_t *>(o.set_pos + item * o.pos_step)[slot] = set_pos;
    reinterpret_cast<uint32_t *>(o.list_pos + item * o.pos_step)[slot] = list_pos;
    uint32_t *c = reinterpret_cast<uint32_t *>(o.common + item * o.common_step) + (size_t)slot * FR_SELECT_EW;
#pragma unroll
    for (int i = 0; i < FR_SELECT_EW; i++) c[i] = w[i];
}

}  // namespace gpbc
#endif
