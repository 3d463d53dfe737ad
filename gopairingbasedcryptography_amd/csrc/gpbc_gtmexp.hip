// libgpbc_bn254.so, unit 8 of 8: reductions in GT — the segmented multi-exponentiation out[s] = prod_i x[i]^k[i] and the plain
// segmented product (csrc/gtmexp29.hip.hpp) with their C-ABI entries (include/gpbc_bn254.h).  gfx950 only.
#include "gpbc_common.hpp"
#include "gtmexp29.hip.hpp"

// What a lane pair works on: piece P = piece0 + (pair of the launch) is piece P % J of segment P / J; its factors come from the
// segment table (every offset clamped to n: a bad table shortens segments, it never reaches outside x) or, for the folds, from
// segments of one length m.  With a shared exponent list a segment ends after nk factors at the latest (the list is never overrun).
struct MexpArgs {
    const uint8_t *x, *k;                 // k: null = product only
    size_t nk;
    int k_shared;                         // 1: k holds one list of nk exponents for every segment
    const uint64_t *seg_off;              // null: uniform segments of m factors
    size_t m, n, n_seg, J, piece0, n_pieces;
    uint8_t *out;                         // piece results, 384 bytes each, at index piece0 + pair
};
__device__ __forceinline__ bool mexp_piece(const MexpArgs &g, size_t pair, size_t &lo, size_t &a, size_t &b, size_t &P) {
    if (pair >= g.n_pieces) return false;
    P = g.piece0 + pair;
    const size_t s = P / g.J;
    size_t hi;
    if (g.seg_off) {
        const uint64_t o0 = g.seg_off[s], o1 = g.seg_off[s + 1];
        lo = o0 < g.n ? (size_t)o0 : g.n;
        hi = o1 < g.n ? (size_t)o1 : g.n;
        if (hi < lo) hi = lo;
    } else { lo = s * g.m; hi = lo + g.m; }
    if (g.k && g.k_shared && hi - lo > g.nk) hi = lo + g.nk;
    gt_mexp_piece_range(lo, hi, P % g.J, g.J, a, b);
    return true;
}
GPBC_KERNEL k_gt_multi_exp(MexpArgs g, int32_t *__restrict__ tabws) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    size_t lo, a, b, P;
    if (!mexp_piece(g, lane >> 1, lo, a, b, P)) return;
    const PairDpp px{(bool)(lane & 1)};
    const size_t half = px.odd ? 192 : 0, k0 = g.k_shared ? lo : 0;
    const uint32_t *kw = reinterpret_cast<const uint32_t *>(g.k);
    F6 r = f12p_multi_exp(px, b - a, [&](size_t i) { return f6_load(g.x + (a + i) * GPBC_GT_BYTES + half); },
                          [&](size_t i, int w) { return (int)((kw[(a + i - k0) * 8 + (w >> 3)] >> (4 * (w & 7))) & 15); },
                          tabws + lane * (size_t)GT_MEXP_TAB_DWORDS);
    f6_store(g.out + P * GPBC_GT_BYTES + half, r);
}
GPBC_KERNEL k_gt_prod(MexpArgs g) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    size_t lo, a, b, P;
    if (!mexp_piece(g, lane >> 1, lo, a, b, P)) return;
    const PairDpp px{(bool)(lane & 1)};
    const size_t half = px.odd ? 192 : 0;
    F6 r = f12p_product(px, b - a, [&](size_t i) { return f6_load(g.x + (a + i) * GPBC_GT_BYTES + half); });
    f6_store(g.out + P * GPBC_GT_BYTES + half, r);
}

// ---- host side.  One level = every segment cut into J pieces (J from the sizes alone, gt_mexp_pieces), one lane pair per piece,
// at most GT_MEXP_CHUNK pieces per launch (their window tables are the bulk of the workspace); J > 1 leaves n_seg x J piece values,
// which the next level folds as uniform segments of J factors in product-only mode, and so on until J = 1 writes `out`.
constexpr size_t GT_MEXP_CHUNK = GT_MEXP_FILL;
constexpr size_t GT_MEXP_TAB_BYTES = 2 * (size_t)GT_MEXP_TAB_DWORDS * sizeof(int32_t);      // per piece: both lanes of the pair
struct MexpPlan { size_t tab_bytes, val_bytes[2]; };
// workspace layout: [tables | piece values of the odd levels | piece values of the even levels]
static MexpPlan mexp_plan(size_t n, size_t n_seg, bool has_k) {
    MexpPlan p{0, {0, 0}};
    if (!n_seg) return p;
    size_t J = gt_mexp_pieces(n, n_seg, has_k);
    if (has_k) { const size_t pieces = n_seg * J; p.tab_bytes = Scratch::padded((pieces < GT_MEXP_CHUNK ? pieces : GT_MEXP_CHUNK) * GT_MEXP_TAB_BYTES); }
    for (int level = 0; J > 1; level++) {
        const size_t pieces = n_seg * J, bytes = Scratch::padded(pieces * GPBC_GT_BYTES);
        if (p.val_bytes[level & 1] < bytes) p.val_bytes[level & 1] = bytes;
        J = gt_mexp_pieces(pieces, n_seg, false);
    }
    return p;
}
static size_t plan_bytes(const MexpPlan &p) { return p.tab_bytes + p.val_bytes[0] + p.val_bytes[1]; }

extern "C" {

size_t gpbc_gt_multi_exp_workspace_bytes(size_t n, size_t n_seg) {
    const size_t a = plan_bytes(mexp_plan(n, n_seg, true)), b = plan_bytes(mexp_plan(n, n_seg, false));
    return a > b ? a : b;
}
// the argument rules shared by the host and the device entry (everything that needs no look at a table)
static int mexp_check_args(const void *x, const void *k, size_t nk, const void *seg_off, size_t n, size_t n_seg, const void *out) {
    if (!n_seg) return fail(GPBC_ERR_INVALID_ARG, "invalid inputs sizes");
    if (!seg_off) return fail(GPBC_ERR_INVALID_ARG, "null segment table");
    if ((n && !x) || !out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    if (!k && nk) return fail(GPBC_ERR_INVALID_ARG, "nk must be 0 without exponents (got nk = %zu)", nk);
    if (k && nk != n && (nk > n || nk * n_seg != n))
        return fail(GPBC_ERR_INVALID_ARG, "nk must be n, or n / n_seg when every segment has that many elements (got nk = %zu, n = %zu, n_seg = %zu)", nk, n, n_seg);
    const uint8_t *xb = (const uint8_t *)x, *ob = (const uint8_t *)out;
    if (n && xb < ob + n_seg * GPBC_GT_BYTES && ob < xb + n * GPBC_GT_BYTES) return fail(GPBC_ERR_INVALID_ARG, "out must not overlap x");
    return GPBC_OK;
}
int gpbc_gt_multi_exp_dev(const void *d_x, const void *d_k, size_t nk, const uint64_t *d_seg_off, size_t n, size_t n_seg,
                          void *d_out, void *d_workspace, size_t workspace_bytes, void *stream) {
    TRY(mexp_check_args(d_x, d_k, nk, d_seg_off, n, n_seg, d_out));
    const MexpPlan plan = mexp_plan(n, n_seg, d_k != nullptr);
    if (plan_bytes(plan) && (!d_workspace || workspace_bytes < plan_bytes(plan)))
        return fail(GPBC_ERR_INVALID_ARG, "workspace too small: %zu bytes given, %zu needed (gpbc_gt_multi_exp_workspace_bytes)", workspace_bytes, plan_bytes(plan));
    TRY(bind_device());
    const hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)d_workspace;
    int32_t *tabws = (int32_t *)ws;
    uint8_t *val[2] = {ws + plan.tab_bytes, ws + plan.tab_bytes + plan.val_bytes[0]};
    MexpArgs g{(const uint8_t *)d_x, (const uint8_t *)d_k, nk, d_k && nk != n, d_seg_off, 0, n, n_seg, 0, 0, 0, nullptr};
    for (int level = 0;; level++) {
        g.J = gt_mexp_pieces(g.n, n_seg, g.k != nullptr);
        g.out = g.J > 1 ? val[level & 1] : (uint8_t *)d_out;
        const size_t pieces = n_seg * g.J;
        for (size_t p0 = 0; p0 < pieces; p0 += GT_MEXP_CHUNK) {
            g.piece0 = p0;
            g.n_pieces = pieces - p0 < GT_MEXP_CHUNK ? pieces - p0 : GT_MEXP_CHUNK;
            if (g.k) TRY(GPBC_LAUNCH(k_gt_multi_exp, grid_for(2 * g.n_pieces), BLOCK, st, g, tabws));
            else TRY(GPBC_LAUNCH(k_gt_prod, grid_for(2 * g.n_pieces), BLOCK, st, g));
        }
        if (g.J == 1) return GPBC_OK;
        g = MexpArgs{g.out, nullptr, 0, 0, nullptr, g.J, pieces, n_seg, 0, 0, 0, nullptr};      // fold: n_seg segments of J piece values each
    }
}
// Host-pointer entry: the table is validated here; segments are the independent units, so a shard is a run of whole segments with
// its table rebased to zero (as gpbc_multi_pair cuts), each through host_call: a call of up to SMALL_CALL_MAX_UNITS elements on a
// call lane of its own (not combined), a larger one through device blocks.
int gpbc_gt_multi_exp(const void *x, const void *k, size_t nk, const uint64_t *seg_off, size_t n_seg, void *out) {
    if (!n_seg) return fail(GPBC_ERR_INVALID_ARG, "invalid inputs sizes");
    if (!seg_off) return fail(GPBC_ERR_INVALID_ARG, "null segment table");
    if (seg_off[0] != 0) return fail(GPBC_ERR_INVALID_ARG, "seg_off[0] must be 0");
    for (size_t j = 0; j < n_seg; j++)
        if (seg_off[j + 1] < seg_off[j]) return fail(GPBC_ERR_INVALID_ARG, "segment table not monotone at %zu", j);
    const size_t n = (size_t)seg_off[n_seg];
    TRY(mexp_check_args(x, k, nk, seg_off, n, n_seg, out));
    const bool shared = k && nk != n;
    if (shared)
        for (size_t j = 0; j < n_seg; j++)
            if (seg_off[j + 1] - seg_off[j] != nk) return fail(GPBC_ERR_INVALID_ARG, "a shared exponent list of %zu needs segments of %zu elements (segment %zu has %zu)", nk, nk, j, (size_t)(seg_off[j + 1] - seg_off[j]));
    auto run = [=](const void *xs, const void *ks, size_t nks, const uint64_t *seg, size_t segs, size_t ns, void *o) {
        HostCall c = HostCall().input(xs, ns * GPBC_GT_BYTES, true).input(ks, nks * GPBC_SCALAR_BYTES, true).input(seg, (segs + 1) * sizeof(uint64_t), true).output(o, GPBC_GT_BYTES);
        c.units = ns > segs ? ns : segs;
        const size_t wsb = gpbc_gt_multi_exp_workspace_bytes(ns, segs);
        return host_call(segs, c, HostRoute{CALL_KINDS, nullptr, 0, SMALL_CALL_MAX_UNITS, 0, wsb}, [=](const DevCols &d, size_t, hipStream_t st) {
            return gpbc_gt_multi_exp_dev(d.in[0], d.in[1], nks, (const uint64_t *)d.in[2], ns, segs, d.out[0], d.tmp, wsb, st);
        });
    };
    const size_t avg = n / n_seg ? n / n_seg : 1;
    constexpr size_t SHARD_MIN_ELEMENTS = 4096;
    return run_sharded(n_seg, (SHARD_MIN_ELEMENTS + avg - 1) / avg, [=](size_t lo, size_t hi) {
        if (lo == 0 && hi == n_seg) return run(x, k, nk, seg_off, n_seg, n, out);
        std::vector<uint64_t> sub(hi - lo + 1);
        const uint64_t base = seg_off[lo];
        for (size_t j = lo; j <= hi; j++) sub[j - lo] = seg_off[j] - base;
        const size_t ns = (size_t)sub.back();
        return run((const uint8_t *)x + base * GPBC_GT_BYTES, k && !shared ? (const uint8_t *)k + base * GPBC_SCALAR_BYTES : k, shared ? nk : k ? ns : 0,
                   sub.data(), hi - lo, ns, (uint8_t *)out + lo * GPBC_GT_BYTES);
    });
}

}  // extern "C"
