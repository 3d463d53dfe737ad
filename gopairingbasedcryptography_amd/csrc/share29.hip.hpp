// Secret sharing in Fr for gfx950: polynomial evaluation (utils.ComputePolynomialValue of the reference, as fibe/sw05_fibe_common.go:205-210
// and fibe/sw05_fibe_large_universe.go:153-167 call it once per attribute of a user) and the recursion of AccessTreeNode.ShareSecret
// (access/tree/access_tree_node.go:58-75) under BSW07 Encrypt, for k polynomials / k secrets per call.  Built on fr29.hip.hpp; the
// kernels (k_fr_poly_eval, k_fr_share_tree in csrc/gpbc_fr.hip) and the host harness (tools/bounds_check.cpp) differ only in where
// the staged values wait.
//
// One step of both: carry <- c_i + carry x, x in internal form (x 2^261), c_i and carry plain.  Nothing is made canonical on the way:
// a coefficient waits in LDS as its 32 bytes cut into nine limbs (any value below 2^256 < 5.3 r, limbs 0..7 in [0, 2^29)), the product
// comes out in (-eps r, (1 + eps) r) with limbs 0..7 in [0, 2^29), so the carry's limbs stay below 2^30 and its value below 6.4 r
// however many steps follow, and the next product's columns stay below 9 x 2^59 + 9 x 2^58 < 2^63 (asserted under -DGPBC_BOUNDS).
// Only what is written is made canonical: fr_canonical<1, 7> takes (-r, 7 r).
#ifndef GPBC_SHARE29_HIP_HPP
#define GPBC_SHARE29_HIP_HPP
#include <vector>
#include "fr29.hip.hpp"

namespace gpbc {

constexpr int FR_SHARE_WAVE = 64;
GPBC_INLINE Fr fr_share_step(const Fr &carry, const Fr &c_i, const Fr &x) { return fr_add(c_i, fr_mul(carry, x)); }
GPBC_INLINE Fr fr_share_out(const Fr &v) { return fr_canonical<1, 7>(v); }
// a small integer (a child's position, at most 1024) in internal form
GPBC_INLINE Fr fr_share_position(uint32_t x) {
    Fr p = fr_zero();
    p.l.v[0] = (int32_t)x;
    GPBC_B(p.l.hi[0] = (double)x; p.l.vb = 1.0;)
    return fr_to_internal(p);
}

// ------------------------------------------------------------------------------------------------ polynomial evaluation
// out[j][t] = sum_{i<d} coeffs[j][i] points[j][t]^i.  One wave per workgroup, a lane owns one point and walks Horner from the top
// coefficient.  A row takes m lanes: a wave holds rpb = 64 / m rows with their own coefficients (m < 64), or a row spreads over
// bpr = ceil(m / 64) workgroups.  The coefficients of a workgroup's rows are staged at word (local row) x pitch + i x NL of an LDS block
// of cap x NL + 64 words, cap = 256 or 1024 coefficients; the pitch is odd (lanes of one row read one address: a broadcast; lanes of
// different rows read different banks).  One shared coefficient row (coeff_step == 0) is staged once.
constexpr int FR_EVAL_SMALL = 256, FR_EVAL_LARGE = 1024;
struct PolyEvalGeom { uint32_t d, m, rpb, bpr, large; };
struct PolyEvalLane { size_t row; uint32_t lr, t; bool active; };
inline PolyEvalGeom fr_poly_eval_geometry(size_t d, size_t m, bool shared_coeffs) {
    PolyEvalGeom g;
    g.d = (uint32_t)d; g.m = (uint32_t)m;
    g.bpr = (uint32_t)((m + FR_SHARE_WAVE - 1) / FR_SHARE_WAVE);
    g.rpb = g.bpr > 1 ? 1 : FR_SHARE_WAVE / g.m;
    const size_t need = shared_coeffs ? d : g.rpb * d;
    g.large = need > (size_t)FR_EVAL_SMALL;
    if (need > (size_t)FR_EVAL_LARGE) g.rpb = (uint32_t)((size_t)FR_EVAL_LARGE / d);       // >= 1: d <= 1024
    return g;
}
GPBC_INLINE uint32_t fr_poly_eval_pitch(const PolyEvalGeom &g) { return (g.d * NL) | 1u; }
GPBC_INLINE size_t fr_poly_eval_row0(const PolyEvalGeom &g, uint32_t block) { return (size_t)(block / g.bpr) * g.rpb; }
GPBC_INLINE uint32_t fr_poly_eval_rows(const PolyEvalGeom &g, uint32_t block, size_t k) {
    const size_t left = k - fr_poly_eval_row0(g, block);
    return left < g.rpb ? (uint32_t)left : g.rpb;
}
GPBC_INLINE size_t fr_poly_eval_grid(const PolyEvalGeom &g, size_t k) { return (k + g.rpb - 1) / g.rpb * g.bpr; }
template <class Put> GPBC_INLINE void fr_poly_eval_stage(const PolyEvalGeom &g, uint32_t block, uint32_t lane, size_t k, const uint8_t *coeffs, size_t coeff_step, const Put &put) {
    const size_t row0 = fr_poly_eval_row0(g, block);
    const uint32_t staged = coeff_step ? fr_poly_eval_rows(g, block, k) : 1u, pitch = fr_poly_eval_pitch(g);
    for (uint32_t idx = lane; idx < staged * g.d; idx += FR_SHARE_WAVE) {
        const uint32_t lr = idx / g.d, i = idx % g.d;
        put(lr * pitch + i * NL, fr_load_raw(coeffs + (row0 + lr) * coeff_step + 32 * (size_t)i));
    }
}
GPBC_INLINE PolyEvalLane fr_poly_eval_map(const PolyEvalGeom &g, uint32_t block, uint32_t lane, size_t k) {
    PolyEvalLane l;
    l.lr = g.bpr > 1 ? 0 : lane / g.m;
    l.t = g.bpr > 1 ? (block % g.bpr) * FR_SHARE_WAVE + lane : lane % g.m;
    l.row = fr_poly_eval_row0(g, block) + l.lr;
    l.active = l.lr < fr_poly_eval_rows(g, block, k) && l.t < g.m;
    return l;
}
// coeff_at(i): coefficient i of the lane's row as it was staged
template <class CoeffAt> GPBC_INLINE void fr_poly_eval_lane(const CoeffAt &coeff_at, uint32_t d, const uint8_t *point, uint8_t *out) {
    const Fr x = fr_poly_point(point);
    Fr carry = coeff_at(d - 1);
    for (uint32_t i = d - 1; i-- > 0;) carry = fr_share_step(carry, coeff_at(i), x);
    fr_store_canonical(out, fr_share_out(carry));
}

// ------------------------------------------------------------------------------------------------ sharing over a threshold tree
// The tree as the kernel walks it, made once on the host (fr_share_plan): every node but the root is a UNIT — the evaluation of its
// parent's polynomial q(X) = value + c_1 X + ... + c_(t-1) X^(t-1) at its child position — and the units are ordered by depth, list order
// within a depth.  Gates and leaves are numbered in list order (leaves from 0 here; the reference's ids start at 1); gate g owns the
// coefficients [coef, coef + t_g - 1) of an item's row, the order in which ShareSecret draws them.
constexpr uint32_t FR_SHARE_MAX = 1024;                 // leaves, gates, children of one gate
constexpr uint32_t FR_SHARE_ROOT = 0xffffffffu, FR_SHARE_LEAF = 0x80000000u;
struct ShareNode { uint32_t parent, threshold; };       // gpbc_share_node
struct ShareUnit { uint32_t gate_x, coef_steps, dest, pad; };       // parent gate | position << 16, first coefficient | (t - 1) << 16, leaf | FR_SHARE_LEAF or gate
struct SharePlan {
    uint32_t L = 0, G = 0, C = 0, depth = 0, wmin = 0;   // leaves, gates, coefficients per item, levels below the root, narrowest level
    std::vector<ShareUnit> units;
    std::vector<uint32_t> level_off;                     // depth + 1 offsets into units
};
// 0, or the reason the node list is refused
inline const char *fr_share_plan(const ShareNode *nodes, size_t n, SharePlan &p) {
    if (!nodes || !n) return "a tree needs at least one node";
    if (n > 2 * (size_t)FR_SHARE_MAX) return "more than 1024 leaves or 1024 gates";
    if (nodes[0].parent != FR_SHARE_ROOT) return "node 0 must carry the root marker";
    std::vector<uint32_t> children(n, 0), rank(n, 0), depth(n, 0), number(n, 0), coef(n, 0);
    p = SharePlan();
    for (size_t i = 0; i < n; i++) {
        if (i) {
            const uint32_t par = nodes[i].parent;
            if (par == FR_SHARE_ROOT) return "a second root";
            if (par >= i) return "a parent must come before its children";
            if (!nodes[par].threshold) return "the parent of a node is a leaf";
            rank[i] = ++children[par];
            depth[i] = depth[par] + 1;
            if (depth[i] > p.depth) p.depth = depth[i];
        }
        if (nodes[i].threshold) {
            if (nodes[i].threshold > FR_SHARE_MAX) return "a threshold above 1024";
            number[i] = p.G++;
            coef[i] = p.C;
            p.C += nodes[i].threshold - 1;
        } else {
            number[i] = p.L++;
        }
        if (p.L > FR_SHARE_MAX || p.G > FR_SHARE_MAX) return "more than 1024 leaves or 1024 gates";
    }
    for (size_t i = 0; i < n; i++) {
        if (children[i] > FR_SHARE_MAX) return "more than 1024 children of one gate";
        if (nodes[i].threshold > children[i]) return "a gate's threshold exceeds its number of children";
    }
    p.level_off.assign(p.depth + 1, 0);
    for (size_t i = 1; i < n; i++) p.level_off[depth[i]]++;                 // counts at [1 .. depth]
    uint32_t at = 0;
    p.wmin = p.depth ? FR_SHARE_WAVE : 0;
    std::vector<uint32_t> next(p.depth + 1, 0);
    for (uint32_t lv = 1; lv <= p.depth; lv++) {
        const uint32_t w = p.level_off[lv];
        if (w < p.wmin) p.wmin = w;
        next[lv] = at;
        p.level_off[lv - 1] = at;
        at += w;
    }
    p.level_off[p.depth] = at;
    p.units.resize(at);
    for (size_t i = 1; i < n; i++) {
        const uint32_t par = nodes[i].parent;
        p.units[next[depth[i]]++] = ShareUnit{number[par] | rank[i] << 16, coef[par] | (nodes[par].threshold - 1) << 16,
                                              nodes[i].threshold ? number[i] : number[i] | FR_SHARE_LEAF, 0};
    }
    return nullptr;
}
// whether a sharing unit stays inside a tree of L leaves, G gates and C coefficients per item
inline bool fr_share_unit_ok(const ShareUnit &s, uint32_t L, uint32_t G, uint32_t C) {
    const uint32_t d = s.dest & ~FR_SHARE_LEAF, x = s.gate_x >> 16, c0 = s.coef_steps & 0xffffu, steps = s.coef_steps >> 16;
    return (s.gate_x & 0xffffu) < G && d < ((s.dest & FR_SHARE_LEAF) ? L : G) && x >= 1 && x <= FR_SHARE_MAX && c0 + steps <= C;
}
// whether every index of a plan's records lies inside the table it points into: asked once, before the plan is uploaded or walked, so
// that the kernel can use the records as they are
inline bool fr_share_plan_ok(const SharePlan &p) {
    if (p.level_off.size() != p.depth + 1 || p.units.size() + 1 != (size_t)p.L + p.G) return false;
    if (p.L > FR_SHARE_MAX || p.G > FR_SHARE_MAX || p.G + p.C > 2 * FR_SHARE_MAX || p.level_off[p.depth] != p.units.size()) return false;
    for (uint32_t lv = 0; lv < p.depth; lv++)
        if (p.level_off[lv] > p.level_off[lv + 1]) return false;
    for (const ShareUnit &u : p.units)
        if (!fr_share_unit_ok(u, p.L, p.G, p.C)) return false;
    return true;
}

// What a lane knows of the item it works on, whichever walk hands it out (the single tree's here and in recon29.hip.hpp, the forest's
// in forest29.hip.hpp): the item's first LDS word, its tree's gates and units (U only where there are state words: the weights), and
// item x row width, the item's first column of the per-leaf arrays.  Every LDS offset of an item is formed from it, here.
struct ItemView { uint32_t base, G, U; size_t row; };
GPBC_INLINE uint32_t fr_item_state(const ItemView &v) { return v.base + v.G * NL; }                                       // the item's state word 0
GPBC_INLINE uint32_t fr_item_used(const ItemView &v, uint32_t gate) { return v.base + v.G * NL + v.U + 1 + gate; }
// one sharing unit of an item: the parent's polynomial at the child's position, Horner from the top coefficient, to the leaf's share or the gate's value
template <class Get, class Put> GPBC_INLINE void fr_share_unit(const ItemView &it, const ShareUnit &un, const Get &get, const Put &put, uint8_t *out) {
    const uint32_t gate = un.gate_x & 0xffffu, x = un.gate_x >> 16, c0 = un.coef_steps & 0xffffu, steps = un.coef_steps >> 16;
    Fr v = get(it.base + gate * NL);
    if (steps) {
        const Fr xi = fr_share_position(x);
        const uint32_t cw = it.base + (it.G + c0) * NL;
        Fr carry = get(cw + (steps - 1) * NL);
        for (uint32_t i = steps - 1; i-- > 0;) carry = fr_share_step(carry, get(cw + i * NL), xi);
        v = fr_share_step(carry, v, xi);
    }
    v = fr_share_out(v);
    if (un.dest & FR_SHARE_LEAF) fr_store_canonical(out + 32 * (it.row + (un.dest & ~FR_SHARE_LEAF)), v);
    else put(it.base + un.dest * NL, v);
}

// The launch: one wave per workgroup, ipb items per workgroup.  An item's block in LDS holds its gates' values (gate g at word g x NL;
// gate 0 is the secret) and behind them its coefficients (c at (G + c) x NL), E = G + C elements at an odd pitch; the values stay there
// between levels, so only coefficients in and leaf shares out touch HBM.  At a level of width W the wave's lanes take the ipb x W units
// 64 at a time: lanes on children of one gate read one address (a broadcast), neighbouring leaves are neighbouring lanes (a wave writes
// 2 KB in one piece).  ipb = 64 / (narrowest level), as far as the LDS instance the item needs anyway allows: 272 elements (9.8 KB: sixteen
// workgroups per CU, four waves per SIMD; a 256-of-256 gate needs 256, sixteen 16-of-16 gates under a 16-of-16 gate 272) or 2048 (72 KB).  A tree that is one leaf has no gate: a lane per item, out = secret.
constexpr int FR_TREE_SMALL = 272, FR_TREE_LARGE = 2048;
struct ShareGeom { uint32_t L, G, C, depth, ipb, pitch, large; };
inline ShareGeom fr_share_geometry(const SharePlan &p) {
    ShareGeom g;
    g.L = p.L; g.G = p.G; g.C = p.C; g.depth = p.depth;
    const uint32_t E = p.G + p.C;
    g.pitch = (E * NL) | 1u;
    g.large = E > (uint32_t)FR_TREE_SMALL;
    if (!p.G) { g.ipb = FR_SHARE_WAVE; return g; }
    const uint32_t want = FR_SHARE_WAVE / (p.wmin ? p.wmin : 1), fit = (uint32_t)(g.large ? FR_TREE_LARGE : FR_TREE_SMALL) / E;       // fit >= 1: E <= 2047
    g.ipb = want < 1 ? 1 : want < fit ? want : fit;
    return g;
}
GPBC_INLINE size_t fr_share_grid(const ShareGeom &g, size_t k) { return (k + g.ipb - 1) / g.ipb; }
GPBC_INLINE uint32_t fr_share_items(const ShareGeom &g, uint32_t block, size_t k) {
    const size_t left = k - (size_t)block * g.ipb;
    return left < g.ipb ? (uint32_t)left : g.ipb;
}
template <class Put> GPBC_INLINE void fr_share_stage(const ShareGeom &g, uint32_t block, uint32_t lane, size_t k, const uint8_t *secrets, const uint8_t *coeffs, const Put &put) {
    if (!g.G) return;
    const size_t item0 = (size_t)block * g.ipb;
    const uint32_t items = fr_share_items(g, block, k), per = g.C + 1;
    for (uint32_t idx = lane; idx < items * per; idx += FR_SHARE_WAVE) {
        const uint32_t li = idx / per, c = idx % per;
        if (c == 0) put(li * g.pitch, fr_load_raw(secrets + 32 * (item0 + li)));
        else put(li * g.pitch + (g.G + c - 1) * NL, fr_load_raw(coeffs + 32 * ((item0 + li) * g.C + (c - 1))));
    }
}
// a lane's share of level lv (1 .. depth); a barrier belongs after it
template <class Get, class Put>
GPBC_INLINE void fr_share_level(const ShareGeom &g, const ShareUnit *units, const uint32_t *level_off, uint32_t lv, uint32_t block, uint32_t lane, size_t k, const Get &get,
                                const Put &put, uint8_t *out) {
    const size_t item0 = (size_t)block * g.ipb;
    const uint32_t first = level_off[lv - 1], W = level_off[lv] - first, total = fr_share_items(g, block, k) * W;
    for (uint32_t u = lane; u < total; u += FR_SHARE_WAVE) {
        const uint32_t li = u / W;
        fr_share_unit(ItemView{li * g.pitch, g.G, 0, (item0 + li) * g.L}, units[first + u % W], get, put, out);
    }
}
// the tree that is one leaf
GPBC_INLINE void fr_share_single(uint32_t block, uint32_t lane, size_t k, const uint8_t *secrets, uint8_t *out) {
    const size_t item = (size_t)block * FR_SHARE_WAVE + lane;
    if (item < k) fr_store_canonical(out + 32 * item, fr_share_out(fr_load_raw(secrets + 32 * item)));
}

}  // namespace gpbc
#endif
