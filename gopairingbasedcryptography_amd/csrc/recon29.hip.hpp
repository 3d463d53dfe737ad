// Reconstruction weights of a threshold tree in Fr for gfx950: the other half of share29.hip.hpp's fr_share_tree.  For k attribute sets
// over one tree, w[j][y] with sum_y w[j][y] share_y = secret for every sharing of the tree: AccessTreeNode.DecryptNode of the reference
// (access/tree/access_tree_node.go:96-164) with the Lagrange coefficients multiplied down each leaf's path instead of applied as GT
// exponents gate by gate — what bsw07.decrypt_plan computes in Python integers for one attribute set.  The definition is theirs:
//   a leaf is satisfied iff it is held; a gate iff at least `threshold` children are; a satisfied gate USES its first `threshold`
//   satisfied children in child order, at positions S; the used child at position i takes the factor
//   Delta_{i,S}(0) = prod_{j in S, j != i} (0 - j) / (i - j); a used leaf's weight is the product of the factors on its path from the root;
//   every other leaf gets 0; an unsatisfied root gives ok = 0 and a zero row; a tree that is one leaf gives w = 1 when held.
// Built on fr29.hip.hpp and on share29.hip.hpp's plan (its checks, its numbering of leaves and gates, its level widths); the kernel (k_fr_tree_weights in csrc/gpbc_fr.hip) and
// the host harness (tools/bounds_check.cpp) differ only in where the staged values wait.
//
// Two passes over the levels.  UP, from the deepest gates to the root, a lane per (item, gate): it walks the gate's children — neighbours
// in the plan's unit order, which numbers the nodes breadth first — counts the
// satisfied ones, marks the first `threshold` CHOSEN and, with `threshold` of them, itself SAT.  DOWN, from the root's children to the
// leaves, a lane per (item, unit): a unit is used iff its parent gate is used and it is chosen; a used unit walks its parent's chosen
// list and multiplies numerator prod j and denominator prod (j - i) over the positions j != i of the list, the numerator starting at
// the parent's weight.  The positions are plain small integers — two of them multiplied in one limb first, so a pair of positions
// costs one product on either side — and nothing is converted: as in fr_lagrange_lane numerator and
// denominator take the same number of plain factors, so the powers of 2^261 cancel in the quotient, and as there a lane owns
// FR_RECON_G units and inverts the product of their denominators once.  A gate's weight waits in LDS in internal form (x 2^261, the
// nine limbs of a product as they are), so a child's numerator starts there unconverted; only leaf weights are made canonical.
#ifndef GPBC_RECON29_HIP_HPP
#define GPBC_RECON29_HIP_HPP
#include <vector>
#include "share29.hip.hpp"

namespace gpbc {

constexpr int FR_RECON_WAVE = 64, FR_RECON_G = FR_LAGRANGE_G;
constexpr uint32_t FR_RECON_SAT = 1, FR_RECON_CHOSEN = 2;
struct ReconGate { uint32_t slot, first, n_t, number; };    // its state word (0: the root, 1 + unit), first child unit, children | threshold << 16, gate number
struct ReconUnit { uint32_t gate_x, dest, sib, pad; };      // parent gate | position << 16, leaf | FR_SHARE_LEAF or gate, parent's first child unit | children << 16
struct ReconPlan {
    uint32_t L = 0, G = 0, U = 0, depth = 0, wmin = 0;       // leaves, gates, units (nodes below the root), levels below the root, narrowest level
    std::vector<ReconUnit> units;                            // by depth; within a depth by parent (in the parents' order), then by position
    std::vector<uint32_t> level_off;                         // depth + 1 offsets into units (SharePlan's: the levels are as wide there)
    std::vector<ReconGate> gates;                            // by depth, in the units' order
    std::vector<uint32_t> gate_off;                          // depth + 1 offsets into gates: the gates at depth lv are [gate_off[lv], gate_off[lv + 1])
};
// 0, or the reason the node list is refused: fr_share_plan's reasons and no other, so every list that can be shared over can be
// reconstructed over.  The units are numbered breadth first — a gate's children follow each other in child order whatever the order of
// the list (the list only needs parent < child; in depth-first preorder this is share29's unit order).
inline const char *fr_recon_plan(const ShareNode *nodes, size_t n, ReconPlan &r) {
    SharePlan p;
    if (const char *why = fr_share_plan(nodes, n, p)) return why;
    r = ReconPlan();
    r.L = p.L; r.G = p.G; r.U = (uint32_t)p.units.size(); r.depth = p.depth; r.wmin = p.wmin; r.level_off = p.level_off;
    std::vector<uint32_t> children(n, 0), rank(n, 0), depth(n, 0), number(n, 0), unit(n, 0), first(n, 0), kid_off(n + 1, 0), kids(n ? n - 1 : 0), queue;
    uint32_t leaves = 0, gates = 0;
    for (size_t i = 0; i < n; i++) {
        if (i) {
            rank[i] = ++children[nodes[i].parent];
            depth[i] = depth[nodes[i].parent] + 1;
        }
        number[i] = nodes[i].threshold ? gates++ : leaves++;
    }
    for (size_t i = 0; i < n; i++) kid_off[i + 1] = kid_off[i] + children[i];
    for (size_t i = 1; i < n; i++) kids[kid_off[nodes[i].parent] + rank[i] - 1] = (uint32_t)i;
    queue.reserve(n);
    queue.push_back(0);
    for (size_t at = 0; at < queue.size(); at++) {           // breadth first: queue position - 1 is the unit
        const uint32_t node = queue[at];
        for (uint32_t c = kid_off[node]; c < kid_off[node + 1]; c++) {
            unit[kids[c]] = (uint32_t)queue.size() - 1;
            if (c == kid_off[node]) first[node] = unit[kids[c]];
            queue.push_back(kids[c]);
        }
    }
    r.gate_off.assign(p.depth + 2, 0);
    for (size_t i = 0; i < n; i++)
        if (nodes[i].threshold) r.gate_off[depth[i] + 1]++;  // a gate has a child, so depth[i] < p.depth
    for (uint32_t lv = 0; lv <= p.depth; lv++) r.gate_off[lv + 1] += r.gate_off[lv];
    r.gate_off.resize(p.depth + 1);                          // the last entry would be G again
    std::vector<uint32_t> gnext(r.gate_off);
    r.units.resize(r.U);
    r.gates.resize(r.G);
    for (uint32_t node : queue) {
        if (node) {
            const uint32_t par = nodes[node].parent;
            r.units[unit[node]] = ReconUnit{number[par] | rank[node] << 16, nodes[node].threshold ? number[node] : number[node] | FR_SHARE_LEAF, first[par] | children[par] << 16, 0};
        }
        if (nodes[node].threshold) r.gates[gnext[depth[node]]++] = ReconGate{node ? 1 + unit[node] : 0, first[node], children[node] | nodes[node].threshold << 16, number[node]};
    }
    return nullptr;
}
// whether a reconstruction unit, resp. a gate, stays inside a tree of L leaves, G gates and U units
inline bool fr_recon_unit_ok(const ReconUnit &u, uint32_t L, uint32_t G, uint32_t U) {
    const uint32_t d = u.dest & ~FR_SHARE_LEAF, sf = u.sib & 0xffffu, nc = u.sib >> 16, x = u.gate_x >> 16;
    return (u.gate_x & 0xffffu) < G && d < ((u.dest & FR_SHARE_LEAF) ? L : G) && sf + nc <= U && x >= 1 && x <= nc;
}
inline bool fr_recon_gate_ok(const ReconGate &q, uint32_t G, uint32_t U) {
    const uint32_t nc = q.n_t & 0xffffu, t = q.n_t >> 16;
    return q.slot <= U && q.number < G && q.first + nc <= U && t >= 1 && t <= nc;
}
// whether every index of a plan's records lies inside the table it points into, as fr_share_plan_ok
inline bool fr_recon_plan_ok(const ReconPlan &p) {
    if (p.units.size() != p.U || p.gates.size() != p.G || p.level_off.size() != p.depth + 1 || p.gate_off.size() != p.depth + 1) return false;
    if (p.L > FR_SHARE_MAX || p.G > FR_SHARE_MAX || p.U + 1 != p.L + p.G) return false;
    if (p.depth && (p.level_off[p.depth] != p.U || p.gate_off[p.depth] != p.G)) return false;
    for (uint32_t lv = 0; lv < p.depth; lv++)
        if (p.level_off[lv] > p.level_off[lv + 1] || p.gate_off[lv] > p.gate_off[lv + 1]) return false;
    for (const ReconUnit &u : p.units)
        if (!fr_recon_unit_ok(u, p.L, p.G, p.U)) return false;
    for (const ReconGate &q : p.gates)
        if (!fr_recon_gate_ok(q, p.G, p.U)) return false;
    return true;
}

// The launch: one wave per workgroup, ipb items per workgroup.  An item's block in LDS, at an odd pitch: its gates' weights (gate g at
// word g x NL; gate 0 is the root, weight 1), behind them U + 1 state words (word 0 the root's, word 1 + u unit u's: SAT | CHOSEN) and G
// words that say whether gate g is used.  A state word is written by the staging, then by the one lane that walks its parent (UP); a
// used word by the lane of the gate's own unit one level before its children read it (DOWN; the root's by UP's last level).
// ipb = 256 / (narrowest level), so that a level fills the FR_RECON_G units of every lane, at most 64 and as many as fit: 2560 words
// (10 KB; a 256-of-256 gate needs 267, sixteen 16-of-16 gates under a 16-of-16 gate 443) or the largest tree's 12289 (48 KB).
constexpr int FR_RECON_SMALL = 2560, FR_RECON_LARGE = (int)FR_SHARE_MAX * (NL + 3) + 1;
struct ReconGeom { uint32_t L, G, U, depth, ipb, pitch, large; };
inline ReconGeom fr_recon_geometry(const ReconPlan &p) {
    ReconGeom g;
    g.L = p.L; g.G = p.G; g.U = p.U; g.depth = p.depth;
    g.pitch = (p.G * NL + p.U + 1 + p.G) | 1u;              // <= 1024 x 9 + 2048 + 1024, odd: <= FR_RECON_LARGE
    g.large = g.pitch > (uint32_t)FR_RECON_SMALL;
    if (!p.G) { g.ipb = FR_RECON_WAVE; return g; }
    const uint32_t wmin = p.wmin ? p.wmin : 1, chunk = FR_RECON_WAVE * FR_RECON_G;
    const uint32_t want = (chunk + wmin - 1) / wmin, fit = (uint32_t)(g.large ? FR_RECON_LARGE : FR_RECON_SMALL) / g.pitch;      // fit >= 1
    g.ipb = want < fit ? want : fit;
    if (g.ipb > (uint32_t)FR_RECON_WAVE) g.ipb = FR_RECON_WAVE;
    return g;
}
GPBC_INLINE size_t fr_recon_grid(const ReconGeom &g, size_t k) { return (k + g.ipb - 1) / g.ipb; }
GPBC_INLINE uint32_t fr_recon_items(const ReconGeom &g, uint32_t block, size_t k) {
    const size_t left = k - (size_t)block * g.ipb;
    return left < g.ipb ? (uint32_t)left : g.ipb;
}
// item li of the workgroup whose first item is item0, as the shared lane code takes it
GPBC_INLINE ItemView fr_recon_item(const ReconGeom &g, size_t item0, uint32_t li) { return ItemView{li * g.pitch, g.G, g.U, (item0 + li) * g.L}; }
// a plain value of one limb: a position, a difference of two, or the product of two of either (|v| <= 1024 x 1024)
constexpr int32_t FR_RECON_SMALL_MAX = (int32_t)(FR_SHARE_MAX * FR_SHARE_MAX);
GPBC_INLINE Fr fr_recon_small(int32_t v) {
    Fr p = fr_zero();
    p.l.v[0] = v;
    GPBC_B(p.l.lo[0] = -(double)FR_RECON_SMALL_MAX; p.l.hi[0] = (double)FR_RECON_SMALL_MAX; p.l.vb = 1.0; p.lob = 1.0;)
    return p;
}
// a lane's share of the staging: the state words (a leaf's: SAT iff its byte of held is non-zero) and the root's weight
template <class Put, class PutW>
GPBC_INLINE void fr_recon_stage(const ReconGeom &g, const ReconUnit *units, uint32_t block, uint32_t lane, size_t k, const uint8_t *held, const Put &put, const PutW &putw) {
    const size_t item0 = (size_t)block * g.ipb;
    const uint32_t items = fr_recon_items(g, block, k), per = g.U + 1;
    for (uint32_t idx = lane; idx < items * per; idx += FR_RECON_WAVE) {
        const uint32_t s = idx % per;
        const ItemView it = fr_recon_item(g, item0, idx / per);
        uint32_t v = 0;
        if (s == 0) put(it.base, fr_one());
        else {
            const uint32_t dest = units[s - 1].dest;
            if (dest & FR_SHARE_LEAF) v = held[it.row + (dest & ~FR_SHARE_LEAF)] ? FR_RECON_SAT : 0u;
        }
        putw(fr_item_state(it) + s, v);
    }
}
// UP, one gate of an item: count its satisfied children, mark the first `threshold` CHOSEN and, with as many, itself SAT; *ok is the item's ok byte
template <class GetW, class PutW> GPBC_INLINE void fr_recon_gate_up(const ItemView &it, const ReconGate &gt, const GetW &getw, const PutW &putw, uint8_t *ok) {
    const uint32_t n = gt.n_t & 0xffffu, t = gt.n_t >> 16, sb = fr_item_state(it);
    uint32_t cnt = 0;
    for (uint32_t c = 0; c < n && cnt < t; c++) {
        const uint32_t w = sb + 1 + gt.first + c, s = getw(w);
        if (s & FR_RECON_SAT) { putw(w, s | FR_RECON_CHOSEN); cnt++; }
    }
    const bool sat = cnt == t;
    if (sat) putw(sb + gt.slot, FR_RECON_SAT);
    if (!gt.slot) {                                         // the root: used iff satisfied
        putw(fr_item_used(it, gt.number), sat ? 1u : 0u);
        *ok = sat ? 1 : 0;
    }
}
// UP, a lane's share of the gates at depth lv (depth - 1 .. 0); a barrier belongs after it
template <class GetW, class PutW>
GPBC_INLINE void fr_recon_up(const ReconGeom &g, const ReconGate *gates, const uint32_t *gate_off, uint32_t lv, uint32_t block, uint32_t lane, size_t k, const GetW &getw,
                             const PutW &putw, uint8_t *ok_out) {
    const size_t item0 = (size_t)block * g.ipb;
    const uint32_t first = gate_off[lv], W = gate_off[lv + 1] - first, total = fr_recon_items(g, block, k) * W;
    for (uint32_t u = lane; u < total; u += FR_RECON_WAVE) {
        const uint32_t li = u / W;
        fr_recon_gate_up(fr_recon_item(g, item0, li), gates[first + u % W], getw, putw, ok_out + item0 + li);
    }
}
// DOWN, the GG units of a lane that share one inversion.  slot(q): whether the lane has a q-th unit in this batch, which unit of `units`
// it is (its state word is 1 + unit) and which item it belongs to.
struct ReconSlot { bool live; uint32_t unit; ItemView item; };
template <int GG, class Slot, class Get, class Put, class GetW, class PutW>
GPBC_INLINE void fr_recon_down_batch(const ReconUnit *units, const Slot &slot, const Get &get, const Put &put, const GetW &getw, const PutW &putw, uint8_t *w_out) {
    static_assert(GG >= 1 && GG <= 32, "one used bit per unit of a lane");
    Fr Wv[GG], D[GG], P = fr_one();
    uint32_t used = 0;
#pragma unroll
    for (int q = 0; q < GG; q++) {
        const ReconSlot sl = slot(q);
        Fr n = fr_one(), d = fr_one();
        if (sl.live) {
            const uint32_t ui = sl.unit, sb = fr_item_state(sl.item);
            const ReconUnit un = units[ui];
            const uint32_t gate = un.gate_x & 0xffffu, x = un.gate_x >> 16, sfirst = un.sib & 0xffffu, nch = un.sib >> 16;
            if (getw(fr_item_used(sl.item, gate)) && (getw(sb + 1 + ui) & FR_RECON_CHOSEN)) {
                used |= 1u << q;
                n = get(sl.item.base + gate * NL);
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
        const ReconSlot sl = slot(q);
        if (sl.live) {
            const uint32_t dest = units[sl.unit].dest;
            const bool on = (used >> q) & 1u;
            const Fr v = on ? fr_mul(Wv[q], inv) : fr_zero();                             // the plain weight
            if (dest & FR_SHARE_LEAF) fr_store_canonical(w_out + 32 * (sl.item.row + (dest & ~FR_SHARE_LEAF)), on ? fr_canonical<1, 2>(v) : v);
            else {
                if (on) put(sl.item.base + dest * NL, fr_to_internal(v));
                putw(fr_item_used(sl.item, dest), on ? 1u : 0u);
            }
        }
        if (q) inv = fr_mul(inv, D[q]);
    }
}
// DOWN, a lane's share of level lv (1 .. depth); a barrier belongs after it
template <int GG, class Get, class Put, class GetW, class PutW>
GPBC_INLINE void fr_recon_down(const ReconGeom &g, const ReconUnit *units, const uint32_t *level_off, uint32_t lv, uint32_t block, uint32_t lane, size_t k, const Get &get,
                               const Put &put, const GetW &getw, const PutW &putw, uint8_t *w_out) {
    const size_t item0 = (size_t)block * g.ipb;
    const uint32_t first = level_off[lv - 1], W = level_off[lv] - first, total = fr_recon_items(g, block, k) * W;
    for (uint32_t base = 0; base < total; base += FR_RECON_WAVE * GG) {
        const auto slot = [&](int q) {
            const uint32_t u = base + (uint32_t)q * FR_RECON_WAVE + lane;
            return u < total ? ReconSlot{true, first + u % W, fr_recon_item(g, item0, u / W)} : ReconSlot{false, 0, ItemView{0, 0, 0, 0}};
        };
        fr_recon_down_batch<GG>(units, slot, get, put, getw, putw, w_out);
    }
}
// the tree that is one leaf
GPBC_INLINE void fr_recon_single(uint32_t block, uint32_t lane, size_t k, const uint8_t *held, uint8_t *w_out, uint8_t *ok_out) {
    const size_t item = (size_t)block * FR_RECON_WAVE + lane;
    if (item >= k) return;
    const bool h = held[item] != 0;
    fr_store_canonical(w_out + 32 * item, h ? fr_plain_one() : fr_zero());
    ok_out[item] = h ? 1 : 0;
}

}  // namespace gpbc
#endif
