// Boolean formulas as LSSS policies for gfx950: NewLSSSMatrixFromBinaryTree of the reference (access/lsss/lewko_waters_lsss_matrix.go:34-87)
// for k formulas at once, and the 0 / 1 reconstruction weights such a matrix always has.  A formula is a row of int64 codes, the nodes of a
// binary tree in depth-first preorder (gate, left subtree, right subtree): a code >= 0 is a leaf with that attribute, FORMULA_AND and
// FORMULA_OR are gates, FORMULA_END pads the row behind the tree.  Well formed: need = 1; every node takes 1 and a gate adds 2; the tree ends
// where need reaches 0, every later entry is END, no earlier one is END or below FORMULA_OR, and the row does not end with need > 0.
//   BUILD   the root's vector is (1), a counter starts at 1.  An OR hands its vector to both children.  An AND at counter c hands its left
//           child c zeros and -1, its right child its own vector padded to c and then 1; the counter becomes c + 1.  A leaf is the next row.
//           So a vector is a set of +1 columns and at most one -1 column: a 64-bit mask and an index are all its state.
//   SELECT  a leaf is satisfied iff the key holds it, an AND iff both children are, an OR iff either is.  From a satisfied root take both
//           children of an AND and, at an OR, the left child if it is satisfied, else the right: the rows of the leaves reached sum to e_0.
// The codes are untrusted: every stack slot, leaf number and column is checked against its table before it is used.
// The kernels (k_fr_lsss_from_formula, k_formula_select in csrc/gpbc_fr.hip) and the host harnesses (tools/bounds_check.cpp,
// tools/formula_san.cpp) differ only in where the staged words wait.  This file needs nothing but the integer types.
//
// One wave per workgroup, the items' codes staged in LDS as two words each.  BUILD: one item per workgroup; lane 0 walks it (at most
// 127 steps, the pending right children on a stack in LDS, the leaves' records in LDS), a barrier, then all 64 lanes stream the item's
// rows x cols x 32 bytes out, consecutive lanes on consecutive 16-byte pieces.  SELECT: a lane per item, 16 items per workgroup (64 when
// one formula serves all); the walk keeps everything else in registers — the held leaves, the per-node satisfaction bits (two 64-bit words),
// a stack of bits in one 64-bit word (depth <= 64) and the chosen leaves.
#ifndef GPBC_FORMULA29_HIP_HPP
#define GPBC_FORMULA29_HIP_HPP
#include <stddef.h>
#include <stdint.h>
#ifndef GPBC_INLINE
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GPBC_INLINE __host__ __device__ __forceinline__
#else
#define GPBC_INLINE inline
#endif
#endif

namespace gpbc {

constexpr int FORMULA_WAVE = 64, FORMULA_MAX_NODES = 127, FORMULA_MAX = 64;
constexpr int64_t FORMULA_END = -1, FORMULA_AND = -2, FORMULA_OR = -3;
constexpr uint32_t FORMULA_NO_MINUS = 0xffffffffu;
// an item's LDS words in BUILD: codes, the stack (mask low, mask high, minus per slot), the leaves (the same three words), their attributes
// (two words), the verdict (ok, rows, columns).  SELECT stages codes only, 16 items at an odd pitch: they start in different banks.
constexpr uint32_t FORMULA_CODE_WORDS = 2 * FORMULA_MAX_NODES, FORMULA_STACK0 = FORMULA_CODE_WORDS, FORMULA_LEAF0 = FORMULA_STACK0 + 3 * FORMULA_MAX,
                   FORMULA_ATTR0 = FORMULA_LEAF0 + 3 * FORMULA_MAX, FORMULA_RES0 = FORMULA_ATTR0 + 2 * FORMULA_MAX;
constexpr uint32_t FORMULA_SELECT_IPB = 16, FORMULA_SELECT_PITCH = FORMULA_CODE_WORDS + 1;
constexpr int FORMULA_BUILD_WORDS = FORMULA_RES0 + 3, FORMULA_SELECT_WORDS = FORMULA_SELECT_IPB * FORMULA_SELECT_PITCH;
static_assert(FORMULA_SELECT_PITCH % 2 == 1, "an odd pitch");

struct FormulaGeom { uint32_t n_nodes, rows, cols, ipb, pitch, shared, wide; };
// where BUILD's rows go: item j's matrix at matrix + j x mat_step, its rho at rho + j x rho_step, its two dims at dims + j x dims_step
// (dims may be null), ok + j.  wide (in the geometry): matrix and mat_step are multiples of 16, so a piece is one 128-bit store.
struct FormulaOut { uint8_t *matrix, *rho, *dims, *ok; size_t mat_step, rho_step, dims_step; };
struct alignas(16) FormulaPiece { uint32_t w0, w1, w2, w3; };                     // one 128-bit store

inline FormulaGeom formula_build_geometry(size_t n_nodes, size_t rows, size_t cols, bool wide) {
    return FormulaGeom{(uint32_t)n_nodes, (uint32_t)rows, (uint32_t)cols, 1u, 0u, 0u, wide ? 1u : 0u};      // one item per workgroup, its words from 0
}
inline FormulaGeom formula_select_geometry(size_t n_nodes, size_t rows, bool shared) {
    return FormulaGeom{(uint32_t)n_nodes, (uint32_t)rows, 0u, shared ? (uint32_t)FORMULA_WAVE : FORMULA_SELECT_IPB, shared ? 0u : FORMULA_SELECT_PITCH, shared ? 1u : 0u, 0u};
}
GPBC_INLINE size_t formula_grid(const FormulaGeom &g, size_t k) { return (k + g.ipb - 1) / g.ipb; }
GPBC_INLINE uint32_t formula_items(const FormulaGeom &g, uint32_t block, size_t k) {
    const size_t left = k - (size_t)block * g.ipb;
    return left < g.ipb ? (uint32_t)left : g.ipb;
}
// STAGE, a lane's share of the workgroup's codes: putw(word offset, value)
template <class PutW> GPBC_INLINE void formula_stage(const FormulaGeom &g, uint32_t block, uint32_t lane, size_t k, const int64_t *nodes, const PutW &putw) {
    const size_t item0 = (size_t)block * g.ipb;
    const uint32_t staged = g.shared ? 1u : formula_items(g, block, k);
    for (uint32_t idx = lane; idx < staged * g.n_nodes; idx += FORMULA_WAVE) {
        const uint32_t lr = idx / g.n_nodes, u = idx % g.n_nodes;
        const uint64_t c = (uint64_t)nodes[g.shared ? (size_t)u : (item0 + lr) * g.n_nodes + u];
        putw(lr * g.pitch + 2 * u, (uint32_t)c);
        putw(lr * g.pitch + 2 * u + 1, (uint32_t)(c >> 32));
    }
}
template <class GetW> GPBC_INLINE int64_t formula_code(const GetW &getw, uint32_t base, uint32_t u) {
    return (int64_t)((uint64_t)getw(base + 2 * u) | (uint64_t)getw(base + 2 * u + 1) << 32);
}

// ------------------------------------------------------------------------------------------------ BUILD
// the walk of the workgroup's item, lane 0 alone: leaf records, attributes and the verdict into the LDS words
template <class GetW, class PutW> GPBC_INLINE void formula_build_walk(const FormulaGeom &g, uint32_t block, uint32_t lane, size_t k, const GetW &getw, const PutW &putw) {
    if (lane != 0 || block >= k) return;
    const uint32_t base = 0;
    uint64_t mask = 1;                                                            // the root's vector (1)
    uint32_t minus = FORMULA_NO_MINUS, sp = 0, counter = 1, leaves = 0;
    bool ok = true, done = false;
    const auto push = [&](uint64_t m, uint32_t mi) {                              // sp < FORMULA_MAX: checked by the caller
        const uint32_t at = base + FORMULA_STACK0 + 3 * sp++;
        putw(at, (uint32_t)m); putw(at + 1, (uint32_t)(m >> 32)); putw(at + 2, mi);
    };
    for (uint32_t u = 0; u < g.n_nodes && ok; u++) {
        const int64_t c = formula_code(getw, base, u);
        if (done) { ok = c == FORMULA_END; continue; }                            // behind the tree: padding only
        if (c >= 0) {
            if (leaves >= g.rows || leaves >= (uint32_t)FORMULA_MAX) { ok = false; break; }
            const uint32_t at = base + FORMULA_LEAF0 + 3 * leaves, aa = base + FORMULA_ATTR0 + 2 * leaves;
            putw(at, (uint32_t)mask); putw(at + 1, (uint32_t)(mask >> 32)); putw(at + 2, minus);
            putw(aa, (uint32_t)(uint64_t)c); putw(aa + 1, (uint32_t)((uint64_t)c >> 32));
            leaves++;
            if (!sp) { done = true; continue; }
            const uint32_t top = base + FORMULA_STACK0 + 3 * --sp;               // the next pending right child
            mask = (uint64_t)getw(top) | (uint64_t)getw(top + 1) << 32;
            minus = getw(top + 2);
        } else if (c == FORMULA_OR) {
            if (sp >= (uint32_t)FORMULA_MAX) { ok = false; break; }
            push(mask, minus);                                                    // both children carry the node's vector
        } else if (c == FORMULA_AND) {
            if (sp >= (uint32_t)FORMULA_MAX || counter >= g.cols || counter >= (uint32_t)FORMULA_MAX) { ok = false; break; }
            push(mask | (uint64_t)1 << counter, minus);                           // right: the node's vector, then 1 in column c
            mask = 0; minus = counter++;                                          // left: -1 in column c and nothing else
        } else {
            ok = false;                                                           // END inside the tree, or no code at all
        }
    }
    ok = ok && done;
    putw(base + FORMULA_RES0, ok ? 1u : 0u);
    putw(base + FORMULA_RES0 + 1, ok ? leaves : 0u);
    putw(base + FORMULA_RES0 + 2, ok ? counter : 0u);
}
// the two 16-byte halves of r - 1, the canonical -1 (little-endian words)
GPBC_INLINE void formula_minus_one(uint32_t w[4], uint32_t half) {
    w[0] = half ? 0x8181585du : 0xf0000000u; w[1] = half ? 0xb85045b6u : 0x43e1f593u;
    w[2] = half ? 0xe131a029u : 0x79b97091u; w[3] = half ? 0x30644e72u : 0x2833e848u;
}
// the write-out of the workgroup's item, all lanes: piece(item, piece number, four words) for every 16-byte piece of the item's rows x cols
// scalars, rho(item, row, attribute) for every row, done(item, ok, rows, columns) once
template <class GetW, class Piece, class Rho, class Done>
GPBC_INLINE void formula_build_write(const FormulaGeom &g, uint32_t block, uint32_t lane, size_t k, const GetW &getw, const Piece &piece, const Rho &rho, const Done &done) {
    if (block >= k) return;
    const size_t item = block;
    const uint32_t per_row = 2 * g.cols, pieces = g.rows * per_row;
    // a lane's pieces are 64 apart: their rows and places in the row follow by additions from the first (one division per lane, none per piece)
    const uint32_t row_step = FORMULA_WAVE / per_row, rem_step = FORMULA_WAVE % per_row;
    uint32_t row = lane / per_row, rem = lane % per_row;
    const bool ok = getw(FORMULA_RES0) != 0;
    const uint32_t nrows = getw(FORMULA_RES0 + 1), ncols = getw(FORMULA_RES0 + 2);
    for (uint32_t p = lane; p < pieces; p += FORMULA_WAVE) {
        const uint32_t col = rem >> 1, half = rem & 1;
        uint32_t w[4] = {0, 0, 0, 0};
        if (ok && row < nrows && row < (uint32_t)FORMULA_MAX) {
            const uint32_t at = FORMULA_LEAF0 + 3 * row;
            const uint64_t m = (uint64_t)getw(at) | (uint64_t)getw(at + 1) << 32;
            if (col == getw(at + 2)) formula_minus_one(w, half);
            else if (!half && (m >> col & 1)) w[0] = 1;
        }
        piece(item, p, w);
        row += row_step; rem += rem_step;
        if (rem >= per_row) { rem -= per_row; row++; }
    }
    for (uint32_t x = lane; x < g.rows; x += FORMULA_WAVE) {
        int64_t a = FORMULA_END;
        if (ok && x < nrows && x < (uint32_t)FORMULA_MAX) a = (int64_t)((uint64_t)getw(FORMULA_ATTR0 + 2 * x) | (uint64_t)getw(FORMULA_ATTR0 + 2 * x + 1) << 32);
        rho(item, x, a);
    }
    if (lane == 0) done(item, ok, nrows, ncols);
}
// the kernel's piece, rho and done: ordinary vector stores into the rows FormulaOut describes
GPBC_INLINE void formula_store_piece(const FormulaGeom &g, const FormulaOut &o, size_t item, uint32_t p, const uint32_t w[4]) {
    uint8_t *at = o.matrix + item * o.mat_step + (size_t)p * 16;
    if (g.wide) {
        *reinterpret_cast<FormulaPiece *>(at) = FormulaPiece{w[0], w[1], w[2], w[3]};
    } else {
        for (int i = 0; i < 16; i++) at[i] = (uint8_t)(w[i >> 2] >> 8 * (i & 3));
    }
}
GPBC_INLINE void formula_store_rho(const FormulaOut &o, size_t item, uint32_t x, int64_t a) { reinterpret_cast<int64_t *>(o.rho + item * o.rho_step)[x] = a; }
GPBC_INLINE void formula_store_done(const FormulaOut &o, size_t item, bool ok, uint32_t nrows, uint32_t ncols) {
    o.ok[item] = ok ? 1 : 0;
    if (o.dims) { uint32_t *d = reinterpret_cast<uint32_t *>(o.dims + item * o.dims_step); d[0] = nrows; d[1] = ncols; }
}

// ------------------------------------------------------------------------------------------------ SELECT
// the lane's item: out(item, ok, the chosen leaves as a 64-bit mask).  held: the item's g.rows bytes.
template <class GetW, class Out> GPBC_INLINE void formula_select_lane(const FormulaGeom &g, uint32_t block, uint32_t lane, size_t k, const GetW &getw, const uint8_t *held, const Out &out) {
    if (lane >= formula_items(g, block, k)) return;
    const size_t item = (size_t)block * g.ipb + lane;
    const uint32_t base = lane * g.pitch;
    uint64_t hm = 0;
    for (uint32_t x = 0; x < g.rows && x < (uint32_t)FORMULA_MAX; x++)
        if (held[item * g.rows + x]) hm |= (uint64_t)1 << x;
    // the shape: where the tree ends and how many leaves it has
    uint32_t need = 1, leaves = 0, end = 0;
    bool ok = true;
    for (uint32_t u = 0; u < g.n_nodes && u < (uint32_t)FORMULA_MAX_NODES; u++) {
        const int64_t c = formula_code(getw, base, u);
        if (!need) { if (c != FORMULA_END) { ok = false; break; } continue; }
        if (c >= 0) { leaves++; need--; }
        else if (c == FORMULA_AND || c == FORMULA_OR) need++;
        else { ok = false; break; }
        if (!need) end = u + 1;
    }
    ok = ok && !need && leaves <= g.rows && leaves <= (uint32_t)FORMULA_MAX;
    uint64_t chosen = 0, sat0 = 0, sat1 = 0, s = 0;
    // satisfaction, from the last node to the first: a finished subtree's bit waits on the stack; a gate finds its left child's on top
    uint32_t depth = 0, leaf = leaves;
    for (uint32_t u = end; ok && u-- > 0;) {
        const int64_t c = formula_code(getw, base, u);
        uint64_t b;
        if (c >= 0) {
            if (!leaf || depth >= (uint32_t)FORMULA_MAX) { ok = false; break; }
            b = hm >> --leaf & 1;
        } else {
            if (depth < 2) { ok = false; break; }
            const uint64_t l = s & 1, r = s >> 1 & 1;
            s >>= 2; depth -= 2;
            b = c == FORMULA_AND ? l & r : l | r;
        }
        s = s << 1 | b; depth++;
        if (u < 64) sat0 |= b << u; else sat1 |= b << (u - 64);
    }
    ok = ok && (sat0 & 1);
    // the choice, from the first node to the last: `sel` says whether the node is taken, the stack holds the pending right children's
    uint64_t sel = 1;
    s = 0; depth = 0; leaf = 0;
    for (uint32_t u = 0; ok && u < end; u++) {
        const int64_t c = formula_code(getw, base, u);
        if (c >= 0) {
            if (leaf >= (uint32_t)FORMULA_MAX) { ok = false; break; }
            chosen |= sel << leaf++;
            sel = s & 1; s >>= 1;
            if (depth) depth--;
        } else {
            if (depth >= (uint32_t)FORMULA_MAX) { ok = false; break; }
            uint64_t right = sel;
            if (c == FORMULA_OR) {
                const uint32_t v = u + 1;                                         // the left child; v < end <= 127
                const uint64_t ls = v < 64 ? sat0 >> v & 1 : sat1 >> (v - 64 & 63) & 1;
                right = sel & (ls ^ 1);
                sel &= ls;
            }
            s = s << 1 | right; depth++;
        }
    }
    out(item, ok, ok ? chosen : (uint64_t)0);
}
// the kernel's out: the item's row of 0 / 1 bytes and its verdict
GPBC_INLINE void formula_store_chosen(const FormulaGeom &g, uint8_t *chosen_out, uint8_t *ok_out, size_t item, bool ok, uint64_t chosen) {
    for (uint32_t x = 0; x < g.rows; x++) chosen_out[item * g.rows + x] = x < 64 ? (uint8_t)(chosen >> x & 1) : (uint8_t)0;
    ok_out[item] = ok ? 1 : 0;
}

}  // namespace gpbc
#endif
