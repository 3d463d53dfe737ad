// Threshold-tree FORESTS in Fr for gfx950: share29.hip.hpp's sharing and recon29.hip.hpp's reconstruction weights with a tree per item.
// BSW07 encrypts every message under a policy of its own, so the natural batch is k items over T distinct trees: item i names its tree
// in tree_of[i] and one launch serves them all.  Every tree is planned on the host exactly as there (fr_share_plan / fr_recon_plan: the
// same refusals, the same numbering of leaves, gates and coefficients) and the per-tree records are concatenated into one device block:
// the two unit tables (a tree's sharing units and its reconstruction units are as many, so one base serves both), the level offsets,
// the gates and the gate offsets, a header per tree, and the maxima over the forest.  fr_forest_plan_ok checks every index of the block
// before it is uploaded, so the kernels (k_fr_share_forest, k_fr_forest_weights in csrc/gpbc_fr.hip) and the host harness
// (tools/bounds_check.cpp) use the records as they are; the two differ only in where the staged values wait.
//
// The arithmetic is the single-tree kernels': fr_share_step / fr_share_out on unconverted coefficients and positions, the small-integer
// Lagrange products with FR_RECON_G units of a lane sharing one inversion, only what is written made canonical.  What changes is who
// walks what.  The geometry — pitch, items per workgroup, LDS instance — is a function of the forest's maxima alone; an item owns
// lpi = 64 / ipb consecutive lanes of its workgroup's one wave, and at a level its lanes walk the units (or gates) its OWN tree has
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
        for (uint32_t u = 0; u < t.U; u++) {
            const ShareUnit &s = f.sunits[t.units + u];
            const ReconUnit &r = f.runits[t.units + u];
            const uint32_t sd = s.dest & ~FR_SHARE_LEAF, x = s.gate_x >> 16, c0 = s.coef_steps & 0xffffu, steps = s.coef_steps >> 16;
            if ((s.gate_x & 0xffffu) >= t.G || sd >= ((s.dest & FR_SHARE_LEAF) ? t.L : t.G) || x < 1 || x > FR_SHARE_MAX || c0 + steps > t.C) return false;
            const uint32_t rd = r.dest & ~FR_SHARE_LEAF, sf = r.sib & 0xffffu, nc = r.sib >> 16, rx = r.gate_x >> 16;
            if ((r.gate_x & 0xffffu) >= t.G || rd >= ((r.dest & FR_SHARE_LEAF) ? t.L : t.G) || sf + nc > t.U || rx < 1 || rx > nc) return false;
        }
        for (uint32_t g = 0; g < t.G; g++) {
            const ReconGate &q = f.gates[t.gates + g];
            const uint32_t nc = q.n_t & 0xffffu, th = q.n_t >> 16;
            if (q.slot > t.U || q.number >= t.G || q.first + nc > t.U || th < 1 || th > nc) return false;
        }
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
    for (uint32_t u = it.sub; u < W; u += g.lpi) {
        const ShareUnit un = fd.sunits[it.t.units + first + u];
        const uint32_t gate = un.gate_x & 0xffffu, x = un.gate_x >> 16, c0 = un.coef_steps & 0xffffu, steps = un.coef_steps >> 16;
        Fr v = get(it.base + gate * NL);
        if (steps) {
            const Fr xi = fr_share_position(x);
            const uint32_t cw = it.base + (it.t.G + c0) * NL;
            Fr carry = get(cw + (steps - 1) * NL);
            for (uint32_t i = steps - 1; i-- > 0;) carry = fr_share_step(carry, get(cw + i * NL), xi);
            v = fr_share_step(carry, v, xi);
        }
        v = fr_share_out(v);
        if (un.dest & FR_SHARE_LEAF) fr_store_canonical(out + 32 * (it.item * g.Lmax + (un.dest & ~FR_SHARE_LEAF)), v);
        else put(it.base + un.dest * NL, v);
    }
}
// behind the levels: the share of a tree that is one leaf, zeros in the columns the item's tree does not have, the ok byte
GPBC_INLINE void fr_forest_share_finish(const ForestGeom &g, const ForestItem &it, const uint8_t *secrets, uint8_t *out, uint8_t *ok_out) {
    if (!it.live) return;
    if (it.valid && !it.t.G && it.sub == 0) fr_store_canonical(out + 32 * (it.item * g.Lmax), fr_share_out(fr_load_raw(secrets + 32 * it.item)));
    for (uint32_t col = it.t.L + it.sub; col < g.Lmax; col += g.lpi) fr_store_canonical(out + 32 * (it.item * g.Lmax + col), fr_zero());
    if (ok_out && it.sub == 0) ok_out[it.item] = it.valid ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ reconstruction weights
GPBC_INLINE uint32_t fr_forest_state(const ForestItem &it) { return it.base + it.t.G * NL; }                                    // the item's state word 0
GPBC_INLINE uint32_t fr_forest_used(const ForestItem &it, uint32_t gate) { return it.base + it.t.G * NL + it.t.U + 1 + gate; }
template <class Put, class PutW>
GPBC_INLINE void fr_forest_recon_stage(const ForestGeom &g, const ForestItem &it, const ForestDev &fd, const uint8_t *held, const Put &put, const PutW &putw) {
    if (!it.valid || !it.t.G) return;
    for (uint32_t s = it.sub; s < it.t.U + 1; s += g.lpi) {
        uint32_t v = 0;
        if (s == 0) put(it.base, fr_one());
        else {
            const uint32_t dest = fd.runits[it.t.units + s - 1].dest;
            if (dest & FR_SHARE_LEAF) v = held[it.item * g.Lmax + (dest & ~FR_SHARE_LEAF)] ? FR_RECON_SAT : 0u;
        }
        putw(fr_forest_state(it) + s, v);
    }
}
// UP, a lane's share of its tree's gates at depth lv (the forest's depth - 1 .. 0); a barrier belongs after it, for every lane
template <class GetW, class PutW>
GPBC_INLINE void fr_forest_recon_up(const ForestGeom &g, const ForestItem &it, const ForestDev &fd, uint32_t lv, const GetW &getw, const PutW &putw, uint8_t *ok_out) {
    if (!it.valid || lv >= it.t.depth) return;
    const uint32_t first = fd.gate_off[it.t.gate_offs + lv], W = fd.gate_off[it.t.gate_offs + lv + 1] - first, sb = fr_forest_state(it);
    for (uint32_t u = it.sub; u < W; u += g.lpi) {
        const ReconGate gt = fd.gates[it.t.gates + first + u];
        const uint32_t n = gt.n_t & 0xffffu, t = gt.n_t >> 16;
        uint32_t cnt = 0;
        for (uint32_t c = 0; c < n && cnt < t; c++) {
            const uint32_t w = sb + 1 + gt.first + c, s = getw(w);
            if (s & FR_RECON_SAT) { putw(w, s | FR_RECON_CHOSEN); cnt++; }
        }
        const bool sat = cnt == t;
        if (sat) putw(sb + gt.slot, FR_RECON_SAT);
        if (!gt.slot) {                                     // the root: used iff satisfied
            putw(fr_forest_used(it, gt.number), sat ? 1u : 0u);
            ok_out[it.item] = sat ? 1 : 0;
        }
    }
}
// DOWN, a lane's share of level lv (1 .. the forest's depth) of its item's tree; a barrier belongs after it, for every lane
template <int GG, class Get, class Put, class GetW, class PutW>
GPBC_INLINE void fr_forest_recon_down(const ForestGeom &g, const ForestItem &it, const ForestDev &fd, uint32_t lv, const Get &get, const Put &put, const GetW &getw, const PutW &putw,
                                      uint8_t *w_out) {
    static_assert(GG >= 1 && GG <= 32, "one used bit per unit of a lane");
    if (!it.valid || lv > it.t.depth) return;
    const uint32_t first = fd.level_off[it.t.levels + lv - 1], W = fd.level_off[it.t.levels + lv] - first, sb = fr_forest_state(it);
    const ReconUnit *units = fd.runits + it.t.units;
    for (uint32_t b = 0; b < W; b += g.lpi * GG) {
        Fr Wv[GG], D[GG], P = fr_one();
        uint32_t used = 0;
#pragma unroll
        for (int q = 0; q < GG; q++) {
            const uint32_t u = b + (uint32_t)q * g.lpi + it.sub;
            Fr n = fr_one(), d = fr_one();
            if (u < W) {
                const uint32_t ui = first + u;
                const ReconUnit un = units[ui];
                const uint32_t gate = un.gate_x & 0xffffu, x = un.gate_x >> 16, sfirst = un.sib & 0xffffu, nch = un.sib >> 16;
                if (getw(fr_forest_used(it, gate)) && (getw(sb + 1 + ui) & FR_RECON_CHOSEN)) {
                    used |= 1u << q;
                    n = get(it.base + gate * NL);
                    // (0 - j) / (i - j) = j / (j - i); two positions a product: j j' and (j - i)(j' - i) are one limb each
                    int32_t pn = 0, pd = 0;
                    for (uint32_t c = 0; c < nch; c++) {
                        if (c + 1 == x || !(getw(sb + 1 + sfirst + c) & FR_RECON_CHOSEN)) continue;
                        const int32_t j = (int32_t)c + 1, dj = j - (int32_t)x;
                        if (!pn) { pn = j; pd = dj; continue; }
                        n = fr_mul(n, fr_recon_small(pn * j));
                        d = fr_mul(d, fr_recon_small(pd * dj));
                        pn = 0;
                    }
                    if (pn) { n = fr_mul(n, fr_recon_small(pn)); d = fr_mul(d, fr_recon_small(pd)); }
                }
            }
            D[q] = d;
            Wv[q] = q ? fr_mul(n, P) : n;
            P = q ? fr_mul(P, d) : d;
        }
        Fr inv = fr_mul(fr_inv(P), fr_plain_one());            // 2^522 / P / 2^261; no denominator is 0: |j - i| < r
#pragma unroll
        for (int q = GG - 1; q >= 0; q--) {
            const uint32_t u = b + (uint32_t)q * g.lpi + it.sub;
            if (u < W) {
                const uint32_t dest = units[first + u].dest;
                const bool on = (used >> q) & 1u;
                const Fr v = on ? fr_mul(Wv[q], inv) : fr_zero();                             // the plain weight
                if (dest & FR_SHARE_LEAF) fr_store_canonical(w_out + 32 * (it.item * g.Lmax + (dest & ~FR_SHARE_LEAF)), on ? fr_canonical<1, 2>(v) : v);
                else {
                    if (on) put(it.base + dest * NL, fr_to_internal(v));
                    putw(fr_forest_used(it, dest), on ? 1u : 0u);
                }
            }
            if (q) inv = fr_mul(inv, D[q]);
        }
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
