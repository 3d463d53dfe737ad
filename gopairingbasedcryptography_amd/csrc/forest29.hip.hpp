// Threshold-tree FORESTS in Fr for gfx950: share29.hip.hpp's sharing and recon29.hip.hpp's reconstruction weights with a tree per item.
// BSW07 encrypts every message under a policy of its own, so the natural batch is k items over T distinct trees: item i names its tree
// in tree_of[i] and one launch serves them all.  Every tree is planned on the host exactly as there (fr_share_plan / fr_recon_plan: the
// same refusals, the same numbering of leaves, gates and coefficients) and the per-tree records are concatenated into one device block:
// the two unit tables (a tree's sharing units and its reconstruction units are as many, so one base serves both), the level offsets,
// the gates and the gate offsets, a header per tree, and the maxima over the forest.  fr_forest_plan_ok checks every index of the block
// before it is uploaded, so the kernels (k_fr_share_forest, k_fr_forest_weights in csrc/gpbc_fr.hip) and the host harness
// (tools/bounds_check.cpp) use the records as they are; the two differ only in where the staged values wait.
//
// The arithmetic and the LDS offsets are the single-tree kernels' own code: a sharing unit is share29's fr_share_unit, a gate on the way
// UP recon29's fr_recon_gate_up, the FR_RECON_G units of a lane that share one inversion its fr_recon_down_batch, all of them handed the
// item as an ItemView; no field operation is written here.  What is written here is who walks what.  The geometry — pitch, items per
// workgroup, LDS instance — is a function of the forest's maxima alone; an item owns lpi = 64 / ipb consecutive lanes of its workgroup's one wave, and at a level its lanes walk the units (or gates) its OWN tree has
// there, none if its tree is shallower.  The level loops and their barriers run to the forest's deepest tree in every lane.
// Per-item arrays are padded to the maxima: coeffs [k, Cmax] (an item reads its first C_t), held [k, Lmax] (columns >= L_t ignored),
// out and w_out [k, Lmax] (columns >= L_t written as zero).  tree_of[i] >= T: an all-zero row and ok = 0, and no header is read.
#ifndef GPBC_FOREST29_HIP_HPP
#define GPBC_FOREST29_HIP_HPP
#include <vector>
#include "recon29.hip.hpp"

namespace gpbc {

constexpr uint32_t FR_FOREST_MAX_TREES = 65536;
// a tree's sizes and where its records start: units into both unit tables, levels into level_off, gates into gates, gate_offs into gate_off
struct ForestTree { uint32_t L, G, C, U, depth, units, levels, gates, gate_offs, pad[3]; };
struct ForestPlan {
    uint32_t T = 0, Lmax = 0, Gmax = 0, Cmax = 0, Umax = 0, depth_max = 0;
    uint32_t wmin = 0, wmax = 0;                        // narrowest and widest level of any tree (0: no tree has a gate)
    uint32_t Emax = 0, Pmax = 0;                        // LDS per item: most gate values + coefficients (sharing), most words (weights)
    std::vector<ForestTree> trees;
    std::vector<ShareUnit> sunits;
    std::vector<ReconUnit> runits;
    std::vector<uint32_t> level_off, gate_off;          // depth_t + 1 entries per tree each
    std::vector<ReconGate> gates;
};
// 0, or the reason the forest is refused; *bad_tree: the tree the reason belongs to (T: the forest itself).  Tree t is the node list
// nodes[node_off[t] .. node_off[t + 1]), parents counted from the tree's own node 0.
inline const char *fr_forest_plan(const ShareNode *nodes, const uint32_t *node_off, size_t n_trees, ForestPlan &f, size_t *bad_tree) {
    *bad_tree = n_trees;
    if (!n_trees) return "a forest needs at least one tree";
    if (n_trees > (size_t)FR_FOREST_MAX_TREES) return "more than 65536 trees";
    if (!nodes || !node_off) return "null pointer";
    for (size_t t = 0; t < n_trees; t++)
        if (node_off[t + 1] <= node_off[t]) { *bad_tree = t; return "node_off must increase"; }
    f = ForestPlan();
    f.T = (uint32_t)n_trees;
    for (size_t t = 0; t < n_trees; t++) {
        SharePlan sp;
        ReconPlan rp;
        const ShareNode *list = nodes + node_off[t];
        const size_t n = node_off[t + 1] - node_off[t];
        const char *why = fr_share_plan(list, n, sp);
        if (!why) why = fr_recon_plan(list, n, rp);
        if (!why && !fr_recon_plan_ok(rp)) why = "its reconstruction plan points outside its tables";
        if (why) { *bad_tree = t; return why; }
        const ForestTree h{sp.L, sp.G, sp.C, rp.U, sp.depth, (uint32_t)f.sunits.size(), (uint32_t)f.level_off.size(), (uint32_t)f.gates.size(), (uint32_t)f.gate_off.size(), {0, 0, 0}};
        f.trees.push_back(h);
        f.sunits.insert(f.sunits.end(), sp.units.begin(), sp.units.end());
        f.runits.insert(f.runits.end(), rp.units.begin(), rp.units.end());
        f.level_off.insert(f.level_off.end(), sp.level_off.begin(), sp.level_off.end());
        f.gates.insert(f.gates.end(), rp.gates.begin(), rp.gates.end());
        f.gate_off.insert(f.gate_off.end(), rp.gate_off.begin(), rp.gate_off.end());
        const uint32_t E = sp.G + sp.C, P = sp.G * NL + rp.U + 1 + sp.G;
        if (sp.L > f.Lmax) f.Lmax = sp.L;
        if (sp.G > f.Gmax) f.Gmax = sp.G;
        if (sp.C > f.Cmax) f.Cmax = sp.C;
        if (rp.U > f.Umax) f.Umax = rp.U;
        if (sp.depth > f.depth_max) f.depth_max = sp.depth;
        if (E > f.Emax) f.Emax = E;
        if (P > f.Pmax) f.Pmax = P;
        for (uint32_t lv = 1; lv <= sp.depth; lv++) {
            const uint32_t w = sp.level_off[lv] - sp.level_off[lv - 1];
            if (!f.wmin || w < f.wmin) f.wmin = w;
            if (w > f.wmax) f.wmax = w;
        }
    }
    return nullptr;
}
// whether every index of the block lies inside the table it points into and every size below the maxima: asked once, before the block
// is uploaded or walked
inline bool fr_forest_plan_ok(const ForestPlan &f) {
    if (!f.T || f.T > FR_FOREST_MAX_TREES || f.trees.size() != f.T || f.sunits.size() != f.runits.size() || f.level_off.size() != f.gate_off.size()) return false;
    if (f.Lmax > FR_SHARE_MAX || f.Gmax > FR_SHARE_MAX || f.Emax > 2 * FR_SHARE_MAX || f.Pmax >= (uint32_t)FR_RECON_LARGE) return false;
    for (const ForestTree &t : f.trees) {
        if (t.L < 1 || t.L > f.Lmax || t.G > f.Gmax || t.C > f.Cmax || t.U > f.Umax || t.depth > f.depth_max || t.U + 1 != t.L + t.G) return false;
        if (t.G + t.C > f.Emax || t.G * NL + t.U + 1 + t.G > f.Pmax || (!t.G && (t.L != 1 || t.depth))) return false;
        if ((size_t)t.units + t.U > f.sunits.size() || (size_t)t.gates + t.G > f.gates.size()) return false;
        if ((size_t)t.levels + t.depth + 1 > f.level_off.size() || (size_t)t.gate_offs + t.depth + 1 > f.gate_off.size()) return false;
        const uint32_t *lo = f.level_off.data() + t.levels, *go = f.gate_off.data() + t.gate_offs;
        if (t.depth && (lo[0] != 0 || lo[t.depth] != t.U || go[0] != 0 || go[t.depth] != t.G)) return false;
        for (uint32_t lv = 0; lv < t.depth; lv++)
            if (lo[lv] > lo[lv + 1] || go[lv] > go[lv + 1]) return false;
        for (uint32_t u = 0; u < t.U; u++)
            if (!fr_share_unit_ok(f.sunits[t.units + u], t.L, t.G, t.C) || !fr_recon_unit_ok(f.runits[t.units + u], t.L, t.G, t.U)) return false;
        for (uint32_t g = 0; g < t.G; g++)
            if (!fr_recon_gate_ok(f.gates[t.gates + g], t.G, t.U)) return false;
    }
    return true;
}

// The block as the lanes see it, and the launch.  ipb items per workgroup, a power of two: lpi = 64 / ipb lanes per item.  Sharing: an
// item's LDS block is share29's — its gates' values, behind them its coefficients, laid out by its OWN G_t — at the odd pitch of Emax
// elements; ipb = 64 / (narrowest level of the forest) as far as the instance Emax needs allows (FR_TREE_SMALL / FR_TREE_LARGE).
// Weights: recon29's block — gate weights, U_t + 1 state words, G_t used words — at the odd pitch of Pmax words; ipb = 256 / (narrowest
// level) as far as FR_RECON_SMALL / FR_RECON_LARGE allow.  Both rounded down to a power of two, so that an item's lanes are a fixed group.
struct ForestDev {
    const ForestTree *trees;
    const ShareUnit *sunits;
    const ReconUnit *runits;
    const uint32_t *level_off, *gate_off;
    const ReconGate *gates;
};
struct ForestGeom { uint32_t T, Lmax, Cmax, depth, ipb, lpi, pitch, large; };
GPBC_INLINE uint32_t fr_forest_pow2_floor(uint32_t v) {
    uint32_t p = 1;
    while (2 * p <= v) p *= 2;
    return p;
}
inline ForestGeom fr_forest_share_geometry(const ForestPlan &f) {
    ForestGeom g{f.T, f.Lmax, f.Cmax, f.depth_max, (uint32_t)FR_SHARE_WAVE, 1, (f.Emax * NL) | 1u, f.Emax > (uint32_t)FR_TREE_SMALL};
    if (f.Gmax) {
        const uint32_t want = FR_SHARE_WAVE / (f.wmin < (uint32_t)FR_SHARE_WAVE ? f.wmin : FR_SHARE_WAVE), fit = (uint32_t)(g.large ? FR_TREE_LARGE : FR_TREE_SMALL) / f.Emax;     // fit >= 1
        g.ipb = fr_forest_pow2_floor(want < fit ? want : fit);
    }
    g.lpi = FR_SHARE_WAVE / g.ipb;
    return g;
}
inline ForestGeom fr_forest_recon_geometry(const ForestPlan &f) {
    ForestGeom g{f.T, f.Lmax, f.Cmax, f.depth_max, (uint32_t)FR_RECON_WAVE, 1, f.Pmax | 1u, 0};
    g.large = g.pitch > (uint32_t)FR_RECON_SMALL;
    if (f.Gmax) {
        const uint32_t chunk = FR_RECON_WAVE * FR_RECON_G, want = (chunk + f.wmin - 1) / f.wmin, fit = (uint32_t)(g.large ? FR_RECON_LARGE : FR_RECON_SMALL) / g.pitch;     // fit >= 1
        const uint32_t most = want < fit ? want : fit;
        g.ipb = fr_forest_pow2_floor(most < (uint32_t)FR_RECON_WAVE ? most : FR_RECON_WAVE);
    }
    g.lpi = FR_RECON_WAVE / g.ipb;
    return g;
}
GPBC_INLINE size_t fr_forest_grid(const ForestGeom &g, size_t k) { return (k + g.ipb - 1) / g.ipb; }

// what a lane knows of its item: live = the item exists, valid = its tree id is below T (only then was a header read: t is all zero otherwise)
struct ForestItem {
    size_t item;
    uint32_t sub, base;                                 // the lane's rank among the item's lanes; the item's first LDS word
    bool live, valid;
    ForestTree t;
};
GPBC_INLINE ForestItem fr_forest_item(const ForestGeom &g, const ForestTree *trees, const uint32_t *tree_of, uint32_t block, uint32_t lane, size_t k) {
    ForestItem it;
    const uint32_t li = lane / g.lpi;
    it.item = (size_t)block * g.ipb + li;
    it.sub = lane % g.lpi;
    it.base = li * g.pitch;
    it.live = it.item < k;
    it.valid = false;
    it.t = ForestTree{0, 0, 0, 0, 0, 0, 0, 0, 0, {0, 0, 0}};
    if (it.live) {
        const uint32_t id = tree_of[it.item];
        if (id < g.T) { it.valid = true; it.t = trees[id]; }     // the id is checked before any address is formed from it
    }
    return it;
}
// the item as the lane code of share29 / recon29 takes it: laid out by its OWN tree's G and U, its rows Lmax columns wide
GPBC_INLINE ItemView fr_forest_view(const ForestGeom &g, const ForestItem &it) { return ItemView{it.base, it.t.G, it.t.U, it.item * g.Lmax}; }

// ------------------------------------------------------------------------------------------------ sharing
template <class Put> GPBC_INLINE void fr_forest_share_stage(const ForestGeom &g, const ForestItem &it, const uint8_t *secrets, const uint8_t *coeffs, const Put &put) {
    if (!it.valid || !it.t.G) return;
    for (uint32_t c = it.sub; c < it.t.C + 1; c += g.lpi) {
        if (c == 0) put(it.base, fr_load_raw(secrets + 32 * it.item));
        else put(it.base + (it.t.G + c - 1) * NL, fr_load_raw(coeffs + 32 * (it.item * g.Cmax + (c - 1))));
    }
}
// a lane's share of level lv (1 .. the forest's depth) of its item's tree; a barrier belongs after it, for every lane
template <class Get, class Put>
GPBC_INLINE void fr_forest_share_level(const ForestGeom &g, const ForestItem &it, const ForestDev &fd, uint32_t lv, const Get &get, const Put &put, uint8_t *out) {
    if (!it.valid || lv > it.t.depth) return;
    const uint32_t first = fd.level_off[it.t.levels + lv - 1], W = fd.level_off[it.t.levels + lv] - first;
    const ItemView view = fr_forest_view(g, it);
    for (uint32_t u = it.sub; u < W; u += g.lpi) fr_share_unit(view, fd.sunits[it.t.units + first + u], get, put, out);
}
// behind the levels: the share of a tree that is one leaf, zeros in the columns the item's tree does not have, the ok byte
GPBC_INLINE void fr_forest_share_finish(const ForestGeom &g, const ForestItem &it, const uint8_t *secrets, uint8_t *out, uint8_t *ok_out) {
    if (!it.live) return;
    if (it.valid && !it.t.G && it.sub == 0) fr_store_canonical(out + 32 * (it.item * g.Lmax), fr_share_out(fr_load_raw(secrets + 32 * it.item)));
    for (uint32_t col = it.t.L + it.sub; col < g.Lmax; col += g.lpi) fr_store_canonical(out + 32 * (it.item * g.Lmax + col), fr_zero());
    if (ok_out && it.sub == 0) ok_out[it.item] = it.valid ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ reconstruction weights
template <class Put, class PutW>
GPBC_INLINE void fr_forest_recon_stage(const ForestGeom &g, const ForestItem &it, const ForestDev &fd, const uint8_t *held, const Put &put, const PutW &putw) {
    if (!it.valid || !it.t.G) return;
    const ItemView view = fr_forest_view(g, it);
    for (uint32_t s = it.sub; s < it.t.U + 1; s += g.lpi) {
        uint32_t v = 0;
        if (s == 0) put(it.base, fr_one());
        else {
            const uint32_t dest = fd.runits[it.t.units + s - 1].dest;
            if (dest & FR_SHARE_LEAF) v = held[view.row + (dest & ~FR_SHARE_LEAF)] ? FR_RECON_SAT : 0u;
        }
        putw(fr_item_state(view) + s, v);
    }
}
// UP, a lane's share of its tree's gates at depth lv (the forest's depth - 1 .. 0); a barrier belongs after it, for every lane
template <class GetW, class PutW>
GPBC_INLINE void fr_forest_recon_up(const ForestGeom &g, const ForestItem &it, const ForestDev &fd, uint32_t lv, const GetW &getw, const PutW &putw, uint8_t *ok_out) {
    if (!it.valid || lv >= it.t.depth) return;
    const uint32_t first = fd.gate_off[it.t.gate_offs + lv], W = fd.gate_off[it.t.gate_offs + lv + 1] - first;
    const ItemView view = fr_forest_view(g, it);
    for (uint32_t u = it.sub; u < W; u += g.lpi) fr_recon_gate_up(view, fd.gates[it.t.gates + first + u], getw, putw, ok_out + it.item);
}
// DOWN, a lane's share of level lv (1 .. the forest's depth) of its item's tree; a barrier belongs after it, for every lane
template <int GG, class Get, class Put, class GetW, class PutW>
GPBC_INLINE void fr_forest_recon_down(const ForestGeom &g, const ForestItem &it, const ForestDev &fd, uint32_t lv, const Get &get, const Put &put, const GetW &getw, const PutW &putw,
                                      uint8_t *w_out) {
    if (!it.valid || lv > it.t.depth) return;
    const uint32_t first = fd.level_off[it.t.levels + lv - 1], W = fd.level_off[it.t.levels + lv] - first;
    const ItemView view = fr_forest_view(g, it);
    for (uint32_t b = 0; b < W; b += g.lpi * GG) {
        const auto slot = [&](int q) {
            const uint32_t u = b + (uint32_t)q * g.lpi + it.sub;
            return ReconSlot{u < W, first + u, view};
        };
        fr_recon_down_batch<GG>(fd.runits + it.t.units, slot, get, put, getw, putw, w_out);
    }
}
// behind the levels: the tree that is one leaf (1 when held), zeros in the columns the item's tree does not have, ok = 0 for a tree id
// out of range
GPBC_INLINE void fr_forest_recon_finish(const ForestGeom &g, const ForestItem &it, const uint8_t *held, uint8_t *w_out, uint8_t *ok_out) {
    if (!it.live) return;
    if (it.sub == 0 && (!it.valid || !it.t.G)) {
        const bool h = it.valid && held[it.item * g.Lmax] != 0;
        if (it.valid) fr_store_canonical(w_out + 32 * (it.item * g.Lmax), h ? fr_plain_one() : fr_zero());
        ok_out[it.item] = h ? 1 : 0;
    }
    for (uint32_t col = it.t.L + it.sub; col < g.Lmax; col += g.lpi) fr_store_canonical(w_out + 32 * (it.item * g.Lmax + col), fr_zero());
}

}  // namespace gpbc
#endif
