// libgpbc_bn254.so, one of the units listed in _build.py: reductions in G1 / G2 — the segmented multi-scalar multiplication
// out[s] = sum_i [k_i] P_i and the plain segmented point sum (csrc/gmsm29.hip.hpp) with their C-ABI entries (include/gpbc_bn254_ext.h).
// The plan, the argument rules, the level walk and the host-pointer route are the segmented-reduction driver's (csrc/segred29.hip.hpp,
// segred_dev / segred_host in csrc/gpbc_core.hip); this unit adds the kernels and how to launch them.  gfx950 only.
#include "gpbc_common.hpp"
#include "../../include/gpbc_bn254_ext.h"
#include "gmsm29.hip.hpp"

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
// A lane per piece (segred_piece: clamped table, uniform folds, shared list never overrun), which the interval harness runs too.
template <class F> __device__ __forceinline__ void gmsm_multi_lane(const SegRedArgs &g, int32_t *ws) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    size_t lo, a, b, P;
    if (!segred_piece(g, lane, lo, a, b, P)) return;
    using Pt = GmsmPoint<F>;
    const size_t k0 = g.k_shared ? lo : 0;
    JacP<F> r = gmsm_lane<F>(b - a, [&](size_t i) { return Pt::load(g.x + (a + i) * Pt::BYTES); },
                             [&](size_t i, uint32_t (&k)[8]) { load_scalar(k, g.k + (a + i - k0) * GPBC_SCALAR_BYTES); },
                             ws + lane * (size_t)gmsm_lane_dwords<F>());
    AffP<F> o;
    jac_to_affine(o, r);
    Pt::store(g.out + P * Pt::BYTES, o);
}
template <class F> __device__ __forceinline__ void gmsm_plain_lane(const SegRedArgs &g) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    size_t lo, a, b, P;
    if (!segred_piece(g, lane, lo, a, b, P)) return;
    using Pt = GmsmPoint<F>;
    JacP<F> r = gmsm_sum_lane<F>(b - a, [&](size_t i) { return Pt::load(g.x + (a + i) * Pt::BYTES); });
    AffP<F> o;
    jac_to_affine(o, r);
    Pt::store(g.out + P * Pt::BYTES, o);
}
GPBC_KERNEL k_g1_multi_scalar_mul(SegRedArgs g, int32_t *__restrict__ ws) { gmsm_multi_lane<Fe>(g, ws); }
GPBC_KERNEL k_g2_multi_scalar_mul(SegRedArgs g, int32_t *__restrict__ ws) { gmsm_multi_lane<F2>(g, ws); }
GPBC_KERNEL_G1 k_g1_sum_segments(SegRedArgs g) { gmsm_plain_lane<Fe>(g); }
GPBC_KERNEL k_g2_sum_segments(SegRedArgs g) { gmsm_plain_lane<F2>(g); }

template <class F> static int gmsm_launch(const SegRedArgs &g, int32_t *tabws, hipStream_t st) {
    constexpr bool g2 = GmsmPoint<F>::BYTES == GPBC_G2_BYTES;
    if (g.k && g2) return GPBC_LAUNCH(k_g2_multi_scalar_mul, grid_for(g.n_pieces), BLOCK, st, g, tabws);
    if (g.k) return GPBC_LAUNCH(k_g1_multi_scalar_mul, grid_for(g.n_pieces), BLOCK, st, g, tabws);
    if (g2) return GPBC_LAUNCH(k_g2_sum_segments, grid_for(g.n_pieces), BLOCK, st, g);
    return GPBC_LAUNCH(k_g1_sum_segments, grid_for(g.n_pieces), BLOCK, st, g);
}
// the lane blocks of a launch's pieces are the bulk of the workspace; their rows are read and written 128 bits at a time
template <class F> static const SegRedOp GMSM_OP{GMSM_SHAPE, GmsmPoint<F>::BYTES, sizeof(int32_t) * (size_t)gmsm_lane_dwords<F>(), 16, "terms", "scalars", "scalar", "the bases",
                                                 "gpbc_multi_scalar_mul_workspace_bytes", gmsm_launch<F>};

extern "C" {

int gpbc_ext_version(void) { return 2; }
size_t gpbc_multi_scalar_mul_workspace_bytes(size_t n, size_t n_seg, int is_g2) { return segred_workspace_bytes(is_g2 ? GMSM_OP<F2> : GMSM_OP<Fe>, n, n_seg); }
int gpbc_g1_multi_scalar_mul_dev(const void *d_bases, const void *d_scalars, size_t nk, const uint64_t *d_seg_off, size_t n, size_t n_seg, void *d_out,
                                 void *d_workspace, size_t workspace_bytes, void *stream) {
    return segred_dev(GMSM_OP<Fe>, d_bases, d_scalars, nk, d_seg_off, n, n_seg, d_out, d_workspace, workspace_bytes, stream);
}
int gpbc_g2_multi_scalar_mul_dev(const void *d_bases, const void *d_scalars, size_t nk, const uint64_t *d_seg_off, size_t n, size_t n_seg, void *d_out,
                                 void *d_workspace, size_t workspace_bytes, void *stream) {
    return segred_dev(GMSM_OP<F2>, d_bases, d_scalars, nk, d_seg_off, n, n_seg, d_out, d_workspace, workspace_bytes, stream);
}
int gpbc_g1_multi_scalar_mul(const void *bases, const void *scalars, size_t nk, const uint64_t *seg_off, size_t n_seg, void *out) {
    return segred_host(GMSM_OP<Fe>, bases, scalars, nk, seg_off, n_seg, out);
}
int gpbc_g2_multi_scalar_mul(const void *bases, const void *scalars, size_t nk, const uint64_t *seg_off, size_t n_seg, void *out) {
    return segred_host(GMSM_OP<F2>, bases, scalars, nk, seg_off, n_seg, out);
}

}  // extern "C"
