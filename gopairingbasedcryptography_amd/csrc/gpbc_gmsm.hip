// libgpbc_bn254.so, unit 9 of 9: reductions in G1 / G2 — the segmented multi-scalar multiplication out[s] = sum_i [k_i] P_i and the
// plain segmented point sum (csrc/gmsm29.hip.hpp) with their C-ABI entries (include/gpbc_bn254_ext.h).  gfx950 only.
#include "gpbc_common.hpp"
#include "../../include/gpbc_bn254_ext.h"
#include "gmsm29.hip.hpp"

// What a lane works on: piece P = piece0 + (lane of the launch) is piece P % J of segment P / J; the segment's range is
// gmsm_segment_range's (clamped table, uniform folds, shared list never overrun), which the interval harness runs too.
struct GmsmArgs {
    const uint8_t *pts, *k;               // k: null = plain sums
    size_t nk;
    int k_shared;                         // 1: k holds one list of nk scalars for every segment
    const uint64_t *seg_off;              // null: uniform segments of m points
    size_t m, n, n_seg, J, piece0, n_pieces;
    uint8_t *out;                         // piece results, one affine point each, at index piece0 + lane
};
__device__ __forceinline__ bool gmsm_piece(const GmsmArgs &g, size_t lane, size_t &lo, size_t &a, size_t &b, size_t &P) {
    if (lane >= g.n_pieces) return false;
    P = g.piece0 + lane;
    size_t hi;
    gmsm_segment_range(g.seg_off, g.m, g.n, P / g.J, g.k && g.k_shared ? g.nk : 0, lo, hi);
    gmsm_piece_range(lo, hi, P % g.J, g.J, a, b);
    return true;
}
template <class F> struct GmsmPoint;
template <> struct GmsmPoint<Fe> {
    static constexpr size_t BYTES = GPBC_G1_BYTES;
    static __device__ __forceinline__ AffP<Fe> load(const uint8_t *p) { return g1_load_aff(p); }
    static __device__ __forceinline__ void store(uint8_t *p, const AffP<Fe> &r) { g1_store_aff(p, r); }
};
template <> struct GmsmPoint<F2> {
    static constexpr size_t BYTES = GPBC_G2_BYTES;
    static __device__ __forceinline__ AffP<F2> load(const uint8_t *p) { return g2_load_aff(p); }
    static __device__ __forceinline__ void store(uint8_t *p, const AffP<F2> &r) { g2_store_aff(p, r); }
};
template <class F> __device__ __forceinline__ void gmsm_multi_lane(const GmsmArgs &g, int32_t *ws) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    size_t lo, a, b, P;
    if (!gmsm_piece(g, lane, lo, a, b, P)) return;
    using Pt = GmsmPoint<F>;
    const size_t k0 = g.k_shared ? lo : 0;
    JacP<F> r = gmsm_lane<F>(b - a, [&](size_t i) { return Pt::load(g.pts + (a + i) * Pt::BYTES); },
                             [&](size_t i, uint32_t (&k)[8]) { load_scalar(k, g.k + (a + i - k0) * GPBC_SCALAR_BYTES); },
                             ws + lane * (size_t)gmsm_lane_dwords<F>());
    AffP<F> o;
    jac_to_affine(o, r);
    Pt::store(g.out + P * Pt::BYTES, o);
}
template <class F> __device__ __forceinline__ void gmsm_plain_lane(const GmsmArgs &g) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    size_t lo, a, b, P;
    if (!gmsm_piece(g, lane, lo, a, b, P)) return;
    using Pt = GmsmPoint<F>;
    JacP<F> r = gmsm_sum_lane<F>(b - a, [&](size_t i) { return Pt::load(g.pts + (a + i) * Pt::BYTES); });
    AffP<F> o;
    jac_to_affine(o, r);
    Pt::store(g.out + P * Pt::BYTES, o);
}
GPBC_KERNEL k_g1_multi_scalar_mul(GmsmArgs g, int32_t *__restrict__ ws) { gmsm_multi_lane<Fe>(g, ws); }
GPBC_KERNEL k_g2_multi_scalar_mul(GmsmArgs g, int32_t *__restrict__ ws) { gmsm_multi_lane<F2>(g, ws); }
GPBC_KERNEL_G1 k_g1_sum_segments(GmsmArgs g) { gmsm_plain_lane<Fe>(g); }
GPBC_KERNEL k_g2_sum_segments(GmsmArgs g) { gmsm_plain_lane<F2>(g); }

// ---- host side.  One level = every segment cut into J pieces (J from the sizes alone, gmsm_pieces), one lane per piece, at most
// GMSM_CHUNK pieces per launch (their tables are the bulk of the workspace); J > 1 leaves n_seg x J piece values, which the next
// level folds as uniform segments of J points in plain-sum mode, and so on until J = 1 writes `out`.
constexpr size_t GMSM_CHUNK = GMSM_FILL;
static size_t gmsm_point_bytes(bool g2) { return g2 ? GPBC_G2_BYTES : GPBC_G1_BYTES; }
static size_t gmsm_block_bytes(bool g2) { return sizeof(int32_t) * (g2 ? (size_t)gmsm_lane_dwords<F2>() : (size_t)gmsm_lane_dwords<Fe>()); }
struct GmsmPlan { size_t tab_bytes, val_bytes[2]; };
// workspace layout: [lane blocks | piece values of the odd levels | piece values of the even levels]
static GmsmPlan gmsm_plan(size_t n, size_t n_seg, bool has_k, bool g2) {
    GmsmPlan p{0, {0, 0}};
    if (!n_seg) return p;
    size_t J = gmsm_pieces(n, n_seg, has_k);
    if (has_k) { const size_t pieces = n_seg * J; p.tab_bytes = Scratch::padded((pieces < GMSM_CHUNK ? pieces : GMSM_CHUNK) * gmsm_block_bytes(g2)); }
    for (int level = 0; J > 1; level++) {
        const size_t pieces = n_seg * J, bytes = Scratch::padded(pieces * gmsm_point_bytes(g2));
        if (p.val_bytes[level & 1] < bytes) p.val_bytes[level & 1] = bytes;
        J = gmsm_pieces(pieces, n_seg, false);
    }
    return p;
}
static size_t plan_bytes(const GmsmPlan &p) { return p.tab_bytes + p.val_bytes[0] + p.val_bytes[1]; }
// the argument rules shared by the host and the device entry (everything that needs no look at a table)
static int gmsm_check_args(bool g2, const void *pts, const void *k, size_t nk, const void *seg_off, size_t n, size_t n_seg, const void *out) {
    if (!n_seg) return fail(GPBC_ERR_INVALID_ARG, "invalid inputs sizes");
    if (!seg_off) return fail(GPBC_ERR_INVALID_ARG, "null segment table");
    if ((n && !pts) || !out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    if (!k && nk) return fail(GPBC_ERR_INVALID_ARG, "nk must be 0 without scalars (got nk = %zu)", nk);
    if (k && nk != n && (nk > n || nk * n_seg != n))
        return fail(GPBC_ERR_INVALID_ARG, "nk must be n, or n / n_seg when every segment has that many terms (got nk = %zu, n = %zu, n_seg = %zu)", nk, n, n_seg);
    const size_t pt = gmsm_point_bytes(g2);
    const uint8_t *pb = (const uint8_t *)pts, *kb = (const uint8_t *)k, *ob = (const uint8_t *)out;
    if (n && pb < ob + n_seg * pt && ob < pb + n * pt) return fail(GPBC_ERR_INVALID_ARG, "out must not overlap the bases");
    if (k && nk && kb < ob + n_seg * pt && ob < kb + nk * GPBC_SCALAR_BYTES) return fail(GPBC_ERR_INVALID_ARG, "out must not overlap the scalars");
    return GPBC_OK;
}
static int gmsm_dev(bool g2, const void *d_pts, const void *d_k, size_t nk, const uint64_t *d_seg_off, size_t n, size_t n_seg, void *d_out,
                    void *d_workspace, size_t workspace_bytes, void *stream) {
    TRY(gmsm_check_args(g2, d_pts, d_k, nk, d_seg_off, n, n_seg, d_out));
    const GmsmPlan plan = gmsm_plan(n, n_seg, d_k != nullptr, g2);
    if (plan_bytes(plan) && (!d_workspace || workspace_bytes < plan_bytes(plan)))
        return fail(GPBC_ERR_INVALID_ARG, "workspace too small: %zu bytes given, %zu needed (gpbc_multi_scalar_mul_workspace_bytes)", workspace_bytes, plan_bytes(plan));
    if (plan_bytes(plan) && ((uintptr_t)d_workspace & 15))
        return fail(GPBC_ERR_INVALID_ARG, "workspace must be 16-byte aligned (its rows are read and written 128 bits at a time)");
    TRY(bind_device());
    const hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)d_workspace;
    int32_t *tabws = (int32_t *)ws;
    uint8_t *val[2] = {ws + plan.tab_bytes, ws + plan.tab_bytes + plan.val_bytes[0]};
    GmsmArgs g{(const uint8_t *)d_pts, (const uint8_t *)d_k, nk, d_k && nk != n, d_seg_off, 0, n, n_seg, 0, 0, 0, nullptr};
    for (int level = 0;; level++) {
        g.J = gmsm_pieces(g.n, n_seg, g.k != nullptr);
        g.out = g.J > 1 ? val[level & 1] : (uint8_t *)d_out;
        const size_t pieces = n_seg * g.J;
        for (size_t p0 = 0; p0 < pieces; p0 += GMSM_CHUNK) {
            g.piece0 = p0;
            g.n_pieces = pieces - p0 < GMSM_CHUNK ? pieces - p0 : GMSM_CHUNK;
            if (g.k && g2) TRY(GPBC_LAUNCH(k_g2_multi_scalar_mul, grid_for(g.n_pieces), BLOCK, st, g, tabws));
            else if (g.k) TRY(GPBC_LAUNCH(k_g1_multi_scalar_mul, grid_for(g.n_pieces), BLOCK, st, g, tabws));
            else if (g2) TRY(GPBC_LAUNCH(k_g2_sum_segments, grid_for(g.n_pieces), BLOCK, st, g));
            else TRY(GPBC_LAUNCH(k_g1_sum_segments, grid_for(g.n_pieces), BLOCK, st, g));
        }
        if (g.J == 1) return GPBC_OK;
        g = GmsmArgs{g.out, nullptr, 0, 0, nullptr, g.J, pieces, n_seg, 0, 0, 0, nullptr};      // fold: n_seg segments of J piece values each
    }
}
static size_t gmsm_workspace_bytes(size_t n, size_t n_seg, bool g2) {
    const size_t a = plan_bytes(gmsm_plan(n, n_seg, true, g2)), b = plan_bytes(gmsm_plan(n, n_seg, false, g2));
    return a > b ? a : b;
}
// Host-pointer entry: the table is validated here; segments are the independent units, so a shard is a run of whole segments with
// its table rebased to zero (as gpbc_gt_multi_exp cuts), each through host_call: a call of up to SMALL_CALL_MAX_UNITS terms on a
// call lane of its own (not combined), a larger one through device blocks.
static int gmsm_host(bool g2, const void *pts, const void *k, size_t nk, const uint64_t *seg_off, size_t n_seg, void *out) {
    if (!n_seg) return fail(GPBC_ERR_INVALID_ARG, "invalid inputs sizes");
    if (!seg_off) return fail(GPBC_ERR_INVALID_ARG, "null segment table");
    if (seg_off[0] != 0) return fail(GPBC_ERR_INVALID_ARG, "seg_off[0] must be 0");
    for (size_t j = 0; j < n_seg; j++)
        if (seg_off[j + 1] < seg_off[j]) return fail(GPBC_ERR_INVALID_ARG, "segment table not monotone at %zu", j);
    const size_t n = (size_t)seg_off[n_seg];
    TRY(gmsm_check_args(g2, pts, k, nk, seg_off, n, n_seg, out));
    const bool shared = k && nk != n;
    if (shared)
        for (size_t j = 0; j < n_seg; j++)
            if (seg_off[j + 1] - seg_off[j] != nk) return fail(GPBC_ERR_INVALID_ARG, "a shared scalar list of %zu needs segments of %zu terms (segment %zu has %zu)", nk, nk, j, (size_t)(seg_off[j + 1] - seg_off[j]));
    const size_t pt = gmsm_point_bytes(g2);
    auto run = [=](const void *ps, const void *ks, size_t nks, const uint64_t *seg, size_t segs, size_t ns, void *o) {
        HostCall c = HostCall().input(ps, ns * pt, true).input(ks, nks * GPBC_SCALAR_BYTES, true).input(seg, (segs + 1) * sizeof(uint64_t), true).output(o, pt);
        c.units = ns > segs ? ns : segs;
        const size_t wsb = gmsm_workspace_bytes(ns, segs, g2);
        return host_call(segs, c, HostRoute{CALL_KINDS, nullptr, 0, SMALL_CALL_MAX_UNITS, 0, wsb}, [=](const DevCols &d, size_t, hipStream_t st) {
            return gmsm_dev(g2, d.in[0], d.in[1], nks, (const uint64_t *)d.in[2], ns, segs, d.out[0], d.tmp, wsb, st);
        });
    };
    const size_t avg = n / n_seg ? n / n_seg : 1;
    constexpr size_t SHARD_MIN_TERMS = 4096;
    return run_sharded(n_seg, (SHARD_MIN_TERMS + avg - 1) / avg, [=](size_t lo, size_t hi) {
        if (lo == 0 && hi == n_seg) return run(pts, k, nk, seg_off, n_seg, n, out);
        std::vector<uint64_t> sub(hi - lo + 1);
        const uint64_t base = seg_off[lo];
        for (size_t j = lo; j <= hi; j++) sub[j - lo] = seg_off[j] - base;
        const size_t ns = (size_t)sub.back();
        return run((const uint8_t *)pts + base * pt, k && !shared ? (const uint8_t *)k + base * GPBC_SCALAR_BYTES : k, shared ? nk : k ? ns : 0,
                   sub.data(), hi - lo, ns, (uint8_t *)out + lo * pt);
    });
}

extern "C" {

int gpbc_ext_version(void) { return 1; }
size_t gpbc_multi_scalar_mul_workspace_bytes(size_t n, size_t n_seg, int is_g2) { return gmsm_workspace_bytes(n, n_seg, is_g2 != 0); }
int gpbc_g1_multi_scalar_mul_dev(const void *d_bases, const void *d_scalars, size_t nk, const uint64_t *d_seg_off, size_t n, size_t n_seg, void *d_out,
                                 void *d_workspace, size_t workspace_bytes, void *stream) {
    return gmsm_dev(false, d_bases, d_scalars, nk, d_seg_off, n, n_seg, d_out, d_workspace, workspace_bytes, stream);
}
int gpbc_g2_multi_scalar_mul_dev(const void *d_bases, const void *d_scalars, size_t nk, const uint64_t *d_seg_off, size_t n, size_t n_seg, void *d_out,
                                 void *d_workspace, size_t workspace_bytes, void *stream) {
    return gmsm_dev(true, d_bases, d_scalars, nk, d_seg_off, n, n_seg, d_out, d_workspace, workspace_bytes, stream);
}
int gpbc_g1_multi_scalar_mul(const void *bases, const void *scalars, size_t nk, const uint64_t *seg_off, size_t n_seg, void *out) {
    return gmsm_host(false, bases, scalars, nk, seg_off, n_seg, out);
}
int gpbc_g2_multi_scalar_mul(const void *bases, const void *scalars, size_t nk, const uint64_t *seg_off, size_t n_seg, void *out) {
    return gmsm_host(true, bases, scalars, nk, seg_off, n_seg, out);
}

}  // extern "C"
