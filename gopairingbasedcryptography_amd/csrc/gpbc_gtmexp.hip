// libgpbc_bn254.so, one of the units listed in _build.py: reductions in GT — the segmented multi-exponentiation
// out[s] = prod_i x[i]^k[i] and the plain segmented product (csrc/gtmexp29.hip.hpp) with their C-ABI entries (include/gpbc_bn254.h).
// The plan, the argument rules, the level walk and the host-pointer route are the segmented-reduction driver's (csrc/segred29.hip.hpp,
// segred_dev / segred_host in csrc/gpbc_core.hip); this unit adds the kernels and how to launch them.  gfx950 only.
#include "gpbc_common.hpp"
#include "gtmexp29.hip.hpp"

// A lane pair per piece (segred_piece): its factors come from the segment table, every offset clamped to n, or, for the folds, from
// segments of one length; with a shared exponent list a segment ends after nk factors at the latest.
GPBC_KERNEL k_gt_multi_exp(SegRedArgs g, int32_t *__restrict__ tabws) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    size_t lo, a, b, P;
    if (!segred_piece(g, lane >> 1, lo, a, b, P)) return;
    const PairDpp px{(bool)(lane & 1)};
    const size_t half = px.odd ? 192 : 0, k0 = g.k_shared ? lo : 0;
    const uint32_t *kw = reinterpret_cast<const uint32_t *>(g.k);
    F6 r = f12p_multi_exp(px, b - a, [&](size_t i) { return f6_load(g.x + (a + i) * GPBC_GT_BYTES + half); },
                          [&](size_t i, int w) { return (int)((kw[(a + i - k0) * 8 + (w >> 3)] >> (4 * (w & 7))) & 15); },
                          tabws + lane * (size_t)GT_MEXP_TAB_DWORDS);
    f6_store(g.out + P * GPBC_GT_BYTES + half, r);
}
GPBC_KERNEL k_gt_prod(SegRedArgs g) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    size_t lo, a, b, P;
    if (!segred_piece(g, lane >> 1, lo, a, b, P)) return;
    const PairDpp px{(bool)(lane & 1)};
    const size_t half = px.odd ? 192 : 0;
    F6 r = f12p_product(px, b - a, [&](size_t i) { return f6_load(g.x + (a + i) * GPBC_GT_BYTES + half); });
    f6_store(g.out + P * GPBC_GT_BYTES + half, r);
}

static int mexp_launch(const SegRedArgs &g, int32_t *tabws, hipStream_t st) {
    if (g.k) return GPBC_LAUNCH(k_gt_multi_exp, grid_for(2 * g.n_pieces), BLOCK, st, g, tabws);
    return GPBC_LAUNCH(k_gt_prod, grid_for(2 * g.n_pieces), BLOCK, st, g);
}
// the window tables of a launch's pieces are the bulk of the workspace; the kernels do not read it 128 bits at a time, so it has no alignment rule
static const SegRedOp GT_MEXP_OP{GT_MEXP_SHAPE, GPBC_GT_BYTES, GT_MEXP_TAB_BYTES, 1, "elements", "exponents", "exponent", "x", "gpbc_gt_multi_exp_workspace_bytes", mexp_launch};

extern "C" {

size_t gpbc_gt_multi_exp_workspace_bytes(size_t n, size_t n_seg) { return segred_workspace_bytes(GT_MEXP_OP, n, n_seg); }
int gpbc_gt_multi_exp_dev(const void *d_x, const void *d_k, size_t nk, const uint64_t *d_seg_off, size_t n, size_t n_seg,
                          void *d_out, void *d_workspace, size_t workspace_bytes, void *stream) {
    return segred_dev(GT_MEXP_OP, d_x, d_k, nk, d_seg_off, n, n_seg, d_out, d_workspace, workspace_bytes, stream);
}
int gpbc_gt_multi_exp(const void *x, const void *k, size_t nk, const uint64_t *seg_off, size_t n_seg, void *out) {
    return segred_host(GT_MEXP_OP, x, k, nk, seg_off, n_seg, out);
}

}  // extern "C"
