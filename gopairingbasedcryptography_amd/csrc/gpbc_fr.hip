// libgpbc_bn254.so, one of the units listed in _build.py: the scalar field Fr on the device (csrc/fr29.hip.hpp) — elementwise add / sub / mul / neg /
// inverse and the fr.Element conversions on the ABI's scalar format, the two polynomial kernels of the AFP25 / GWWW25 opening
// proofs, the Lagrange basis over a node set per row (SW05 fuzzy IBE) and the LSSS reconstruction weights of a policy per
// ciphertext (Waters11 CP-ABE) — with their C-ABI entries (include/gpbc_bn254.h, "scalar field"), and secret sharing (csrc/share29.hip.hpp):
// polynomial evaluation and the shares of a threshold tree (include/gpbc_bn254_share.h), and LSSS share generation (csrc/lsss29.hip.hpp,
// include/gpbc_bn254_indexed.h), and the reconstruction weights of a threshold tree (csrc/recon29.hip.hpp, include/gpbc_bn254_recon.h),
// and the common attributes of a list and a set (csrc/select29.hip.hpp, include/gpbc_bn254_select.h),
// and LSSS matrices and 0 / 1 weights from boolean formulas (csrc/formula29.hip.hpp, include/gpbc_bn254_formula.h),
// and sharing and weights over a forest of threshold trees, a tree per item (csrc/forest29.hip.hpp, include/gpbc_bn254_forest.h).
// gfx950 only.
#include "gpbc_common.hpp"
#include "fr29.hip.hpp"
#include "share29.hip.hpp"
#include "recon29.hip.hpp"
#include "forest29.hip.hpp"
#include "lsss29.hip.hpp"
#include "select29.hip.hpp"
#include "formula29.hip.hpp"
#include "frdot29.hip.hpp"
#include "../../include/gpbc_bn254_share.h"
#include "../../include/gpbc_bn254_indexed.h"
#include "../../include/gpbc_bn254_recon.h"
#include "../../include/gpbc_bn254_select.h"
#include "../../include/gpbc_bn254_formula.h"
#include "../../include/gpbc_bn254_forest.h"
#include "../../include/gpbc_bn254_verify.h"

// ------------------------------------------------------------------------------------------------ elementwise
// one element per lane (no __restrict__: out may be a, or b)
template <int OP> __device__ __forceinline__ void fr_op_kernel(const uint8_t *a, const uint8_t *b, size_t b_step, uint8_t *out, size_t n) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    fr_op_lane<OP>(a + 32 * i, b + i * b_step, out + 32 * i);
}
GPBC_KERNEL_G1 k_fr_add(const uint8_t *a, const uint8_t *b, size_t b_step, uint8_t *out, size_t n) { fr_op_kernel<FR_ADD>(a, b, b_step, out, n); }
GPBC_KERNEL_G1 k_fr_sub(const uint8_t *a, const uint8_t *b, size_t b_step, uint8_t *out, size_t n) { fr_op_kernel<FR_SUB>(a, b, b_step, out, n); }
GPBC_KERNEL_G1 k_fr_mul(const uint8_t *a, const uint8_t *b, size_t b_step, uint8_t *out, size_t n) { fr_op_kernel<FR_MUL>(a, b, b_step, out, n); }
GPBC_KERNEL_G1 k_fr_neg(const uint8_t *a, const uint8_t *b, size_t b_step, uint8_t *out, size_t n) { fr_op_kernel<FR_NEG>(a, b, b_step, out, n); }
GPBC_KERNEL_G1 k_fr_from_mont(const uint8_t *a, const uint8_t *b, size_t b_step, uint8_t *out, size_t n) { fr_op_kernel<FR_FROM_MONT>(a, b, b_step, out, n); }
GPBC_KERNEL_G1 k_fr_to_mont(const uint8_t *a, const uint8_t *b, size_t b_step, uint8_t *out, size_t n) { fr_op_kernel<FR_TO_MONT>(a, b, b_step, out, n); }
// FR_INV_K elements per lane share one inversion
GPBC_KERNEL_G1 k_fr_inverse(const uint8_t *a, uint8_t *out, size_t n) {
    const size_t T = (n + FR_INV_K - 1) / FR_INV_K, t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= T) return;
    fr_inverse_lane<FR_INV_K>(a, out, n, t, T);
}

// ------------------------------------------------------------------------------------------------ polynomials
__device__ __forceinline__ Fr lds_get(const int32_t *p) {
    Fr x;
#pragma unroll
    for (int i = 0; i < NL; i++) x.l.v[i] = p[i];
    return x;
}
__device__ __forceinline__ void lds_put(int32_t *p, const Fr &x) {
#pragma unroll
    for (int i = 0; i < NL; i++) p[i] = x.l.v[i];
}

// prod_{i<B} (X - roots[j][i]): one workgroup per polynomial, the coefficients in LDS (nine limbs each, an odd pitch: no bank
// conflicts), thread t owns the coefficients t, t + 256, ...  One step per root: every coefficient up to the new degree is read
// with its lower neighbour, a barrier, written, a barrier; coefficients past the current degree are not touched.  The roots are
// converted 64 at a time by the first wave.
constexpr int FR_ROOTS_BLOCK = 256, FR_ROOTS_OWN = (FR_POLY_MAX_B + FR_ROOTS_BLOCK) / FR_ROOTS_BLOCK;     // 5 coefficients per thread at B = 1024
__global__ void __launch_bounds__(FR_ROOTS_BLOCK) k_fr_poly_from_roots(const uint8_t *__restrict__ roots, uint32_t B, uint8_t *__restrict__ coeffs_out) {
    __shared__ int32_t cs[(FR_POLY_MAX_B + 1) * NL];
    __shared__ int32_t rs[64 * NL];
    const uint32_t tid = threadIdx.x;
    const uint8_t *rt = roots + (size_t)blockIdx.x * B * 32;
    uint8_t *out = coeffs_out + (size_t)blockIdx.x * (B + 1) * 32;
    for (uint32_t i = tid; i <= B; i += FR_ROOTS_BLOCK) lds_put(cs + i * NL, i ? fr_zero() : fr_plain_one());
    for (uint32_t s = 0; s < B; s++) {
        if ((s & 63) == 0) {
            if (tid < 64 && s + tid < B) lds_put(rs + tid * NL, fr_poly_neg_root(rt + 32 * (size_t)(s + tid)));
            __syncthreads();
        }
        const Fr nr = lds_get(rs + (s & 63) * NL);
        Fr nw[FR_ROOTS_OWN];
#pragma unroll
        for (int m = 0; m < FR_ROOTS_OWN; m++) {
            const uint32_t i = tid + m * FR_ROOTS_BLOCK;
            if (i <= s + 1) nw[m] = fr_poly_root_step(i ? lds_get(cs + (i - 1) * NL) : fr_zero(), lds_get(cs + i * NL), nr);
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < FR_ROOTS_OWN; m++) {
            const uint32_t i = tid + m * FR_ROOTS_BLOCK;
            if (i <= s + 1) lds_put(cs + i * NL, nw[m]);
        }
        __syncthreads();
    }
    for (uint32_t i = tid; i <= B; i += FR_ROOTS_BLOCK) fr_poly_store(out + 32 * (size_t)i, lds_get(cs + i * NL));
}

// coeffs[j](X) / (X - points[j][i]): one lane per (polynomial, point), one wave per workgroup, 64 points of ONE polynomial per wave.
// f's coefficients wait in LDS in canonical limbs (every lane of the wave reads the same address: a broadcast); a lane walks from
// the top coefficient down, one product per step.  The quotient's coefficients are canonical as they fall out of the step, but a
// lane's row is stride x 32 bytes away from its neighbour's, so they are staged: FR_Q_STEPS steps fill a tile of 64 rows x 256 bytes
// in LDS, which the wave then writes out row by row, 64 lanes = 256 contiguous bytes.  After the last step the remainder decides
// ok; then the wave zeroes the padding columns [B, stride) of its rows and, whole, the rows whose division was not exact.
// Two instances: LDS for B <= 256 (26 KB: six workgroups per CU) and for B <= 1024 (53 KB: two).
constexpr int FR_Q_STEPS = 8, FR_Q_PITCH = FR_Q_STEPS * 8 + 1, FR_Q_SMALL_B = 256;
template <int MAXB> __device__ __forceinline__ void fr_poly_quotients_kernel(const uint8_t *__restrict__ coeffs, const uint8_t *__restrict__ points, uint32_t B, uint32_t blocks_per_poly,
                                                                              size_t stride, uint8_t *__restrict__ q_out, uint8_t *__restrict__ ok_out) {
    __shared__ int32_t cs[(MAXB + 1) * NL];
    __shared__ uint32_t tile[BLOCK * FR_Q_PITCH];
    __shared__ uint32_t oks[BLOCK];
    const uint32_t lane = threadIdx.x, j = blockIdx.x / blocks_per_poly, first = (blockIdx.x % blocks_per_poly) * BLOCK;
    const uint32_t pi = first + lane, rows = B - first < BLOCK ? B - first : BLOCK;
    const bool valid = pi < B;
    const uint8_t *f = coeffs + (size_t)j * (B + 1) * 32;
    for (uint32_t i = lane; i <= B; i += BLOCK) lds_put(cs + i * NL, fr_poly_coeff_in(f + 32 * (size_t)i));
    const Fr point = valid ? fr_poly_point(points + ((size_t)j * B + pi) * 32) : fr_zero();
    __syncthreads();
    uint32_t *q = reinterpret_cast<uint32_t *>(q_out) + ((size_t)j * B + first) * stride * 8;      // row 0 of this wave
    Fr carry = fr_zero();
    for (int g = (int)((B - 1) / FR_Q_STEPS); g >= 0; g--) {
        const uint32_t c_lo = (uint32_t)g * FR_Q_STEPS, ncols = B - c_lo < FR_Q_STEPS ? B - c_lo : FR_Q_STEPS;
        for (int c = (int)ncols - 1; c >= 0; c--) {
            carry = fr_poly_horner_step(carry, lds_get(cs + (c_lo + c + 1) * NL), point);      // quotient coefficient c_lo + c
            uint32_t w[8];
            fr_words(w, carry);
#pragma unroll
            for (int k = 0; k < 8; k++) tile[lane * FR_Q_PITCH + c * 8 + k] = w[k];
        }
        __syncthreads();
        if (ncols == FR_Q_STEPS) {
            for (uint32_t row = 0; row < rows; row++) q[((size_t)row * stride + c_lo) * 8 + lane] = tile[row * FR_Q_PITCH + lane];
        } else {
            const uint32_t run = ncols * 8;
            for (uint32_t idx = lane; idx < rows * run; idx += BLOCK) {
                const uint32_t row = idx / run, w = idx % run;
                q[((size_t)row * stride + c_lo) * 8 + w] = tile[row * FR_Q_PITCH + w];
            }
        }
        __syncthreads();
    }
    const bool ok = valid && fr_limbs_zero(fr_poly_horner_step(carry, lds_get(cs), point));
    oks[lane] = ok ? 1u : 0u;
    if (valid) ok_out[(size_t)j * B + pi] = ok ? 1 : 0;
    __syncthreads();                                            // also: the rows are written before they are zeroed
    for (uint32_t row = 0; row < rows; row++)
        for (size_t w = (oks[row] ? (size_t)B * 8 : 0) + lane; w < stride * 8; w += BLOCK) q[(size_t)row * stride * 8 + w] = 0;
}
__global__ void __launch_bounds__(BLOCK) k_fr_poly_quotients(const uint8_t *__restrict__ coeffs, const uint8_t *__restrict__ points, uint32_t B, uint32_t blocks_per_poly, size_t stride,
                                                             uint8_t *__restrict__ q_out, uint8_t *__restrict__ ok_out) {
    fr_poly_quotients_kernel<FR_Q_SMALL_B>(coeffs, points, B, blocks_per_poly, stride, q_out, ok_out);
}
__global__ void __launch_bounds__(BLOCK) k_fr_poly_quotients_long(const uint8_t *__restrict__ coeffs, const uint8_t *__restrict__ points, uint32_t B, uint32_t blocks_per_poly, size_t stride,
                                                                  uint8_t *__restrict__ q_out, uint8_t *__restrict__ ok_out) {
    fr_poly_quotients_kernel<FR_POLY_MAX_B>(coeffs, points, B, blocks_per_poly, stride, q_out, ok_out);
}

// ------------------------------------------------------------------------------------------------ Lagrange basis
// out[j][t] = prod_{u < B, set[j][u] != nodes[j][t]} (x[j] - set[j][u]) / (nodes[j][t] - set[j][u]): fr_lagrange_lane, one wave per
// workgroup.  A lane owns FR_LAGRANGE_G nodes of one row, so a row takes gpr = ceil(m / G) lanes: a wave holds rpb = 64 / gpr rows
// of different sets (m = 16: sixteen lanes-of-four, 16 rows), or a row spreads over bpr = ceil(gpr / 64) workgroups (m > 256).  The
// workgroup stages the sets of its rows in LDS, canonical, nine limbs each with an odd row pitch (lanes of one row read one address:
// a broadcast; lanes of different rows read different banks); a shared set (set_step == 0) is staged once.  Two instances as for
// the quotients: LDS for 256 set elements (9 KB: the common shapes keep every wave slot) and for 1024 (36 KB).  Geometry, staging
// and lane mapping are fr29.hip.hpp's (fr_lagrange_geometry / _stage / _map), which the host harness runs workgroup by workgroup.
static_assert(FR_LAG_WAVE == BLOCK, "one wave per workgroup");
template <int CAP> __device__ __forceinline__ void fr_lagrange_kernel(const uint8_t *__restrict__ set, size_t set_step, const uint8_t *__restrict__ nodes, size_t node_step,
                                                                       const uint8_t *__restrict__ x, size_t x_step, size_t k, LagrangeGeom gm, uint8_t *__restrict__ out) {
    __shared__ int32_t ss[CAP * NL + BLOCK];
    fr_lagrange_stage(gm, blockIdx.x, threadIdx.x, k, set, set_step, [&](uint32_t off, const Fr &v) { lds_put(ss + off, v); });
    __syncthreads();
    const LagrangeLane l = fr_lagrange_map(gm, blockIdx.x, threadIdx.x, k);
    if (!l.active) return;
    const int32_t *mine = ss + (set_step ? l.lr * fr_lagrange_pitch(gm) : 0u);
    const Fr xc = x ? fr_lagrange_in(x + l.row * x_step) : fr_zero();
    fr_lagrange_lane<FR_LAGRANGE_G>([&](uint32_t u) { return lds_get(mine + u * NL); }, gm.B, nodes ? nodes + l.row * node_step : nullptr, xc, gm.m, l.gi, gm.gpr,
                                    out + l.row * gm.m * 32);
}
GPBC_KERNEL_G1 k_fr_lagrange_basis(const uint8_t *__restrict__ set, size_t set_step, const uint8_t *__restrict__ nodes, size_t node_step, const uint8_t *__restrict__ x,
                                   size_t x_step, size_t k, LagrangeGeom gm, uint8_t *__restrict__ out) {
    fr_lagrange_kernel<FR_LAG_SMALL>(set, set_step, nodes, node_step, x, x_step, k, gm, out);
}
__global__ void __launch_bounds__(BLOCK) k_fr_lagrange_basis_long(const uint8_t *__restrict__ set, size_t set_step, const uint8_t *__restrict__ nodes, size_t node_step, const uint8_t *__restrict__ x,
                                        size_t x_step, size_t k, LagrangeGeom gm, uint8_t *__restrict__ out) {
    fr_lagrange_kernel<FR_LAG_LARGE>(set, set_step, nodes, node_step, x, x_step, k, gm, out);
}

// ------------------------------------------------------------------------------------------------ LSSS reconstruction weights
// w[t] with sum_x w[t][x] M_t[x] = (1, 0, ..., 0) over the held rows of system t: a batched Gauss-Jordan solve over Fr, one wave per
// workgroup, spw = 64 / max(rows + 1, cols) systems per wave, a column of the transposed augmented matrix per lane, the columns in
// LDS.  The arithmetic, the geometry, the staging and the lane mapping are fr29.hip.hpp's (fr_lsss_*), which the host harness runs
// workgroup by workgroup; here are only the LDS block, the ballots and the barriers.  One barrier per unknown: after it the owner
// of the pivot column clears it while everybody tests the next column, which the step before the barrier finished.  Three instances
// by LDS block (fr_lsss_words): 29 KB (three 16 x 16 systems, five workgroups per CU), 80 KB and 146.5 KB (64 x 64, alone on its CU).
static_assert(FR_LSSS_WAVE == BLOCK, "one wave per workgroup");
template <int WORDS> __device__ __forceinline__ void fr_lsss_kernel(const uint8_t *__restrict__ matrix, size_t mat_step, const uint8_t *__restrict__ held, size_t k, LsssGeom gm,
                                                                     uint8_t *__restrict__ w_out, uint8_t *__restrict__ ok_out) {
    __shared__ int32_t ss[WORDS];
    const auto get = [&](uint32_t off) { return lds_get(ss + off); };
    const auto put = [&](uint32_t off, const Fr &v) { lds_put(ss + off, v); };
    fr_lsss_stage(gm, blockIdx.x, threadIdx.x, k, matrix, mat_step, held, put);
    __syncthreads();
    const LsssLane l = fr_lsss_map(gm, blockIdx.x, threadIdx.x, k);
    LsssState s = fr_lsss_begin(gm);
    for (uint32_t c = 0; c < gm.rows; c++) {
        const uint64_t nz = __ballot(fr_lsss_nonzero(gm, l, c, get));
        fr_lsss_step(gm, l, c, nz, s, get, put);
        __syncthreads();
        fr_lsss_clear(gm, l, c, s, put);
    }
    const uint64_t nz = __ballot(fr_lsss_nonzero(gm, l, gm.rows, get));
    fr_lsss_finish(gm, l, nz, s, get, w_out, ok_out);
}
#define GPBC_LSSS_ARGS const uint8_t *__restrict__ matrix, size_t mat_step, const uint8_t *__restrict__ held, size_t k, LsssGeom gm, uint8_t *__restrict__ w_out, uint8_t *__restrict__ ok_out
__global__ void __launch_bounds__(BLOCK) k_fr_lsss_weights(GPBC_LSSS_ARGS) { fr_lsss_kernel<FR_LSSS_WORDS_0>(matrix, mat_step, held, k, gm, w_out, ok_out); }
__global__ void __launch_bounds__(BLOCK) k_fr_lsss_weights_mid(GPBC_LSSS_ARGS) { fr_lsss_kernel<FR_LSSS_WORDS_1>(matrix, mat_step, held, k, gm, w_out, ok_out); }
__global__ void __launch_bounds__(BLOCK) k_fr_lsss_weights_large(GPBC_LSSS_ARGS) { fr_lsss_kernel<FR_LSSS_WORDS_2>(matrix, mat_step, held, k, gm, w_out, ok_out); }

// ------------------------------------------------------------------------------------------------ secret sharing
// out[j][t] = coeffs[j](points[j][t]) and the shares of k secrets over one threshold tree: share29.hip.hpp has the arithmetic, the
// geometry, the staging and the lane mapping (the host harness runs them workgroup by workgroup); here are the LDS blocks and the barriers.
// One wave per workgroup, two LDS instances each.
static_assert(FR_SHARE_WAVE == BLOCK, "one wave per workgroup");
template <int CAP> __device__ __forceinline__ void fr_poly_eval_kernel(const uint8_t *__restrict__ coeffs, size_t coeff_step, const uint8_t *__restrict__ points, size_t point_step, size_t k,
                                                                        PolyEvalGeom gm, uint8_t *__restrict__ out) {
    __shared__ int32_t cs[CAP * NL + BLOCK];
    fr_poly_eval_stage(gm, blockIdx.x, threadIdx.x, k, coeffs, coeff_step, [&](uint32_t off, const Fr &v) { lds_put(cs + off, v); });
    __syncthreads();
    const PolyEvalLane l = fr_poly_eval_map(gm, blockIdx.x, threadIdx.x, k);
    if (!l.active) return;
    const int32_t *mine = cs + (coeff_step ? l.lr * fr_poly_eval_pitch(gm) : 0u);
    fr_poly_eval_lane([&](uint32_t i) { return lds_get(mine + i * NL); }, gm.d, points + l.row * point_step + 32 * (size_t)l.t, out + 32 * (l.row * gm.m + l.t));
}
GPBC_KERNEL_G1 k_fr_poly_eval(const uint8_t *__restrict__ coeffs, size_t coeff_step, const uint8_t *__restrict__ points, size_t point_step, size_t k, PolyEvalGeom gm,
                              uint8_t *__restrict__ out) {
    fr_poly_eval_kernel<FR_EVAL_SMALL>(coeffs, coeff_step, points, point_step, k, gm, out);
}
__global__ void __launch_bounds__(BLOCK) k_fr_poly_eval_long(const uint8_t *__restrict__ coeffs, size_t coeff_step, const uint8_t *__restrict__ points, size_t point_step, size_t k, PolyEvalGeom gm,
                                   uint8_t *__restrict__ out) {
    fr_poly_eval_kernel<FR_EVAL_LARGE>(coeffs, coeff_step, points, point_step, k, gm, out);
}
template <int CAP> __device__ __forceinline__ void fr_share_tree_kernel(const ShareUnit *__restrict__ units, const uint32_t *__restrict__ level_off, const uint8_t *__restrict__ secrets,
                                                                         const uint8_t *__restrict__ coeffs, size_t k, ShareGeom gm, uint8_t *__restrict__ out) {
    __shared__ int32_t ss[CAP * NL + BLOCK];
    if (!gm.G) { fr_share_single(blockIdx.x, threadIdx.x, k, secrets, out); return; }
    const auto get = [&](uint32_t off) { return lds_get(ss + off); };
    const auto put = [&](uint32_t off, const Fr &v) { lds_put(ss + off, v); };
    fr_share_stage(gm, blockIdx.x, threadIdx.x, k, secrets, coeffs, put);
    __syncthreads();
    for (uint32_t lv = 1; lv <= gm.depth; lv++) {
        fr_share_level(gm, units, level_off, lv, blockIdx.x, threadIdx.x, k, get, put, out);
        __syncthreads();
    }
}
GPBC_KERNEL_G1 k_fr_share_tree(const ShareUnit *__restrict__ units, const uint32_t *__restrict__ level_off, const uint8_t *__restrict__ secrets, const uint8_t *__restrict__ coeffs,
                               size_t k, ShareGeom gm, uint8_t *__restrict__ out) {
    fr_share_tree_kernel<FR_TREE_SMALL>(units, level_off, secrets, coeffs, k, gm, out);
}
__global__ void __launch_bounds__(BLOCK) k_fr_share_tree_large(const ShareUnit *__restrict__ units, const uint32_t *__restrict__ level_off, const uint8_t *__restrict__ secrets, const uint8_t *__restrict__ coeffs,
                                     size_t k, ShareGeom gm, uint8_t *__restrict__ out) {
    fr_share_tree_kernel<FR_TREE_LARGE>(units, level_off, secrets, coeffs, k, gm, out);
}

// ------------------------------------------------------------------------------------------------ threshold-tree weights
// w[j][y] with sum_y w[j][y] share_y = secret for the leaves item j holds: recon29.hip.hpp has the arithmetic, the plan, the geometry, the
// staging and both passes; here are the LDS block (gate weights, state words and used words of ipb items) and the barriers.
static_assert(FR_RECON_WAVE == BLOCK, "one wave per workgroup");
template <int CAP> __device__ __forceinline__ void fr_tree_weights_kernel(const ReconUnit *__restrict__ units, const uint32_t *__restrict__ level_off, const ReconGate *__restrict__ gates,
                                                                           const uint32_t *__restrict__ gate_off, const uint8_t *__restrict__ held, size_t k, ReconGeom gm,
                                                                           uint8_t *__restrict__ w_out, uint8_t *__restrict__ ok_out) {
    __shared__ int32_t ss[CAP + BLOCK];
    if (!gm.G) { fr_recon_single(blockIdx.x, threadIdx.x, k, held, w_out, ok_out); return; }
    const auto get = [&](uint32_t off) { return lds_get(ss + off); };
    const auto put = [&](uint32_t off, const Fr &v) { lds_put(ss + off, v); };
    const auto getw = [&](uint32_t off) { return (uint32_t)ss[off]; };
    const auto putw = [&](uint32_t off, uint32_t v) { ss[off] = (int32_t)v; };
    fr_recon_stage(gm, units, blockIdx.x, threadIdx.x, k, held, put, putw);
    __syncthreads();
    for (uint32_t lv = gm.depth; lv-- > 0;) {
        fr_recon_up(gm, gates, gate_off, lv, blockIdx.x, threadIdx.x, k, getw, putw, ok_out);
        __syncthreads();
    }
    for (uint32_t lv = 1; lv <= gm.depth; lv++) {
        fr_recon_down<FR_RECON_G>(gm, units, level_off, lv, blockIdx.x, threadIdx.x, k, get, put, getw, putw, w_out);
        __syncthreads();
    }
}
#define GPBC_RECON_ARGS const ReconUnit *__restrict__ units, const uint32_t *__restrict__ level_off, const ReconGate *__restrict__ gates, const uint32_t *__restrict__ gate_off, \
                        const uint8_t *__restrict__ held, size_t k, ReconGeom gm, uint8_t *__restrict__ w_out, uint8_t *__restrict__ ok_out
GPBC_KERNEL_G1 k_fr_tree_weights(GPBC_RECON_ARGS) { fr_tree_weights_kernel<FR_RECON_SMALL>(units, level_off, gates, gate_off, held, k, gm, w_out, ok_out); }
__global__ void __launch_bounds__(BLOCK) k_fr_tree_weights_large(GPBC_RECON_ARGS) { fr_tree_weights_kernel<FR_RECON_LARGE>(units, level_off, gates, gate_off, held, k, gm, w_out, ok_out); }

// ------------------------------------------------------------------------------------------------ threshold-tree forests
// A tree per item: forest29.hip.hpp has the block, the geometry, the item mapping and the lane code; here are the LDS blocks (those of the
// two single-tree kernels above, at the same instance sizes) and the barriers.  Every lane runs every level loop to the forest's depth
// and arrives at every barrier, whatever the depth of its own item's tree and whether its item exists at all.
template <int CAP> __device__ __forceinline__ void fr_share_forest_kernel(ForestDev fd, const uint32_t *__restrict__ tree_of, const uint8_t *__restrict__ secrets,
                                                                           const uint8_t *__restrict__ coeffs, size_t k, ForestGeom gm, uint8_t *__restrict__ out,
                                                                           uint8_t *__restrict__ ok_out) {
    __shared__ int32_t ss[CAP * NL + BLOCK];
    const auto get = [&](uint32_t off) { return lds_get(ss + off); };
    const auto put = [&](uint32_t off, const Fr &v) { lds_put(ss + off, v); };
    const ForestItem it = fr_forest_item(gm, fd.trees, tree_of, blockIdx.x, threadIdx.x, k);
    fr_forest_share_stage(gm, it, secrets, coeffs, put);
    __syncthreads();
    for (uint32_t lv = 1; lv <= gm.depth; lv++) {
        fr_forest_share_level(gm, it, fd, lv, get, put, out);
        __syncthreads();
    }
    fr_forest_share_finish(gm, it, secrets, out, ok_out);
}
#define GPBC_FOREST_SHARE_ARGS ForestDev fd, const uint32_t *__restrict__ tree_of, const uint8_t *__restrict__ secrets, const uint8_t *__restrict__ coeffs, size_t k, ForestGeom gm, \
                               uint8_t *__restrict__ out, uint8_t *__restrict__ ok_out
GPBC_KERNEL_G1 k_fr_share_forest(GPBC_FOREST_SHARE_ARGS) { fr_share_forest_kernel<FR_TREE_SMALL>(fd, tree_of, secrets, coeffs, k, gm, out, ok_out); }
__global__ void __launch_bounds__(BLOCK) k_fr_share_forest_large(GPBC_FOREST_SHARE_ARGS) { fr_share_forest_kernel<FR_TREE_LARGE>(fd, tree_of, secrets, coeffs, k, gm, out, ok_out); }

template <int CAP> __device__ __forceinline__ void fr_forest_weights_kernel(ForestDev fd, const uint32_t *__restrict__ tree_of, const uint8_t *__restrict__ held, size_t k, ForestGeom gm,
                                                                             uint8_t *__restrict__ w_out, uint8_t *__restrict__ ok_out) {
    __shared__ int32_t ss[CAP + BLOCK];
    const auto get = [&](uint32_t off) { return lds_get(ss + off); };
    const auto put = [&](uint32_t off, const Fr &v) { lds_put(ss + off, v); };
    const auto getw = [&](uint32_t off) { return (uint32_t)ss[off]; };
    const auto putw = [&](uint32_t off, uint32_t v) { ss[off] = (int32_t)v; };
    const ForestItem it = fr_forest_item(gm, fd.trees, tree_of, blockIdx.x, threadIdx.x, k);
    fr_forest_recon_stage(gm, it, fd, held, put, putw);
    __syncthreads();
    for (uint32_t lv = gm.depth; lv-- > 0;) {
        fr_forest_recon_up(gm, it, fd, lv, getw, putw, ok_out);
        __syncthreads();
    }
    for (uint32_t lv = 1; lv <= gm.depth; lv++) {
        fr_forest_recon_down<FR_RECON_G>(gm, it, fd, lv, get, put, getw, putw, w_out);
        __syncthreads();
    }
    fr_forest_recon_finish(gm, it, held, w_out, ok_out);
}
#define GPBC_FOREST_RECON_ARGS ForestDev fd, const uint32_t *__restrict__ tree_of, const uint8_t *__restrict__ held, size_t k, ForestGeom gm, uint8_t *__restrict__ w_out, \
                               uint8_t *__restrict__ ok_out
GPBC_KERNEL_G1 k_fr_forest_weights(GPBC_FOREST_RECON_ARGS) { fr_forest_weights_kernel<FR_RECON_SMALL>(fd, tree_of, held, k, gm, w_out, ok_out); }
__global__ void __launch_bounds__(BLOCK) k_fr_forest_weights_large(GPBC_FOREST_RECON_ARGS) { fr_forest_weights_kernel<FR_RECON_LARGE>(fd, tree_of, held, k, gm, w_out, ok_out); }

// ------------------------------------------------------------------------------------------------ LSSS share generation
// out[j][x] = M_x . v_j: lsss29.hip.hpp has the arithmetic, the geometry, the staging and the lane mapping; here is the LDS block of the
// one shared matrix's row group and the barrier.  mat_step != 0: a matrix per item, read by the lanes that own its rows.
static_assert(FR_LSSS_SHARES_WAVE == BLOCK, "one wave per workgroup");
GPBC_KERNEL_G1 k_fr_lsss_shares(const uint8_t *__restrict__ matrix, size_t mat_step, const uint8_t *__restrict__ vectors, size_t k, LsssSharesGeom gm, uint8_t *__restrict__ out) {
    __shared__ int32_t ms[FR_SHARES_CAP * NL + BLOCK];
    if (!mat_step) {
        fr_lsss_shares_stage(gm, blockIdx.x, threadIdx.x, matrix, [&](uint32_t off, const Fr &v) { lds_put(ms + off, v); });
        __syncthreads();
    }
    const LsssSharesLane l = fr_lsss_shares_map(gm, blockIdx.x, threadIdx.x, k);
    if (!l.active) return;
    const uint8_t *vec = vectors + l.item * gm.cols * GPBC_SCALAR_BYTES;
    uint8_t *o = out + (l.item * gm.rows + l.x) * GPBC_SCALAR_BYTES;
    if (mat_step) {
        const uint8_t *row = matrix + l.item * mat_step + (size_t)l.x * gm.cols * GPBC_SCALAR_BYTES;
        fr_lsss_shares_lane([&](uint32_t c) { return fr_load_raw(row + 32 * (size_t)c); }, gm.cols, vec, o);
    } else {
        const int32_t *mine = ms + l.xr * gm.pitch;
        fr_lsss_shares_lane([&](uint32_t c) { return lds_get(mine + c * NL); }, gm.cols, vec, o);
    }
}

// ------------------------------------------------------------------------------------------------ common attributes
// FindCommonAttributes for k (set, list) items: select29.hip.hpp has the geometry, the staging, the lane map and the four phases; here are
// the LDS block (the staged sets, a pos word and a keep word per list element) and the three barriers.  Two instances by LDS block.
static_assert(FR_SELECT_WAVE == BLOCK, "one wave per workgroup");
template <int WORDS> __device__ __forceinline__ void fr_find_common_kernel(const uint8_t *__restrict__ sets, const uint8_t *__restrict__ lists, size_t k, SelectGeom gm, SelectOut o) {
    __shared__ uint32_t ss[WORDS];
    const auto gete = [&](uint32_t off, int i) { return ss[off + i]; };
    const auto getw = [&](uint32_t off) { return ss[off]; };
    const auto putw = [&](uint32_t off, uint32_t v) { ss[off] = v; };
    fr_select_stage(gm, blockIdx.x, threadIdx.x, k, sets, [&](uint32_t off, const uint32_t (&w)[FR_SELECT_EW]) {
#pragma unroll
        for (int i = 0; i < FR_SELECT_EW; i++) ss[off + i] = w[i];
    });
    __syncthreads();
    fr_select_match(gm, blockIdx.x, threadIdx.x, k, lists, gete, putw);
    __syncthreads();
    fr_select_mark(gm, blockIdx.x, threadIdx.x, k, getw, putw);
    __syncthreads();
    fr_select_pick(gm, blockIdx.x, threadIdx.x, k, gete, getw,
                   [&](size_t item, uint32_t slot, uint32_t sp, uint32_t lp, const uint32_t (&w)[FR_SELECT_EW]) { fr_select_store(o, item, slot, sp, lp, w); },
                   [&](size_t item, bool ok) { o.ok[item] = ok ? 1 : 0; });
}
GPBC_KERNEL_G1 k_fr_find_common(const uint8_t *__restrict__ sets, const uint8_t *__restrict__ lists, size_t k, SelectGeom gm, SelectOut o) {
    fr_find_common_kernel<FR_SELECT_WORDS_SMALL>(sets, lists, k, gm, o);
}
__global__ void __launch_bounds__(BLOCK) k_fr_find_common_large(const uint8_t *__restrict__ sets, const uint8_t *__restrict__ lists, size_t k, SelectGeom gm, SelectOut o) {
    fr_find_common_kernel<FR_SELECT_WORDS_LARGE>(sets, lists, k, gm, o);
}

// ------------------------------------------------------------------------------------------------ formulas
// NewLSSSMatrixFromBinaryTree for k formulas and the 0 / 1 weights of such a matrix: formula29.hip.hpp has the geometry, the staging, the
// walks and the write-out; here are the LDS blocks (the items' codes; for the matrices also a stack, the leaf records and the verdict per
// item) and the barriers.
static_assert(FORMULA_WAVE == BLOCK, "one wave per workgroup");
GPBC_KERNEL_G1 k_fr_lsss_from_formula(const int64_t *__restrict__ nodes, size_t k, FormulaGeom gm, FormulaOut o) {
    __shared__ uint32_t ss[FORMULA_BUILD_WORDS];
    const auto getw = [&](uint32_t off) { return ss[off]; };
    const auto putw = [&](uint32_t off, uint32_t v) { ss[off] = v; };
    formula_stage(gm, blockIdx.x, threadIdx.x, k, nodes, putw);
    __syncthreads();
    formula_build_walk(gm, blockIdx.x, threadIdx.x, k, getw, putw);
    __syncthreads();
    formula_build_write(gm, blockIdx.x, threadIdx.x, k, getw,
                        [&](size_t item, uint32_t p, const uint32_t (&w)[4]) { formula_store_piece(gm, o, item, p, w); },
                        [&](size_t item, uint32_t x, int64_t a) { formula_store_rho(o, item, x, a); },
                        [&](size_t item, bool ok, uint32_t nrows, uint32_t ncols) { formula_store_done(o, item, ok, nrows, ncols); });
}
GPBC_KERNEL_G1 k_formula_select(const int64_t *__restrict__ nodes, const uint8_t *__restrict__ held, size_t k, FormulaGeom gm, uint8_t *__restrict__ chosen_out,
                                uint8_t *__restrict__ ok_out) {
    __shared__ uint32_t ss[FORMULA_SELECT_WORDS];
    formula_stage(gm, blockIdx.x, threadIdx.x, k, nodes, [&](uint32_t off, uint32_t v) { ss[off] = v; });
    __syncthreads();
    formula_select_lane(gm, blockIdx.x, threadIdx.x, k, [&](uint32_t off) { return ss[off]; }, held,
                        [&](size_t item, bool ok, uint64_t chosen) { formula_store_chosen(gm, chosen_out, ok_out, item, ok, chosen); });
}

extern "C" {

// ------------------------------------------------------------------------------------------------ elementwise entries
static int fr_dev(int op, const void *d_a, const void *d_b, size_t nb, size_t n, void *d_out, void *stream) {
    const bool binary = op == FR_ADD || op == FR_SUB || op == FR_MUL;
    if (!n) return GPBC_OK;
    if (!d_a || !d_out || (binary && !d_b)) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    if (binary) TRY(nb_one_or_n(nb, n));
    TRY(bind_device());
    const hipStream_t st = (hipStream_t)stream;
    const uint8_t *a = (const uint8_t *)d_a, *b = binary ? (const uint8_t *)d_b : a;
    uint8_t *o = (uint8_t *)d_out;
    const size_t step = binary && nb == n ? GPBC_SCALAR_BYTES : 0;
    const unsigned grid = grid_for(n);
    switch (op) {
        case FR_ADD: return GPBC_LAUNCH(k_fr_add, grid, BLOCK, st, a, b, step, o, n);
        case FR_SUB: return GPBC_LAUNCH(k_fr_sub, grid, BLOCK, st, a, b, step, o, n);
        case FR_MUL: return GPBC_LAUNCH(k_fr_mul, grid, BLOCK, st, a, b, step, o, n);
        case FR_NEG: return GPBC_LAUNCH(k_fr_neg, grid, BLOCK, st, a, b, step, o, n);
        case FR_FROM_MONT: return GPBC_LAUNCH(k_fr_from_mont, grid, BLOCK, st, a, b, step, o, n);
        case FR_TO_MONT: return GPBC_LAUNCH(k_fr_to_mont, grid, BLOCK, st, a, b, step, o, n);
        default: return GPBC_LAUNCH(k_fr_inverse, grid_for((n + FR_INV_K - 1) / FR_INV_K), BLOCK, st, a, o, n);
    }
}
// Host-pointer entries: sharded over the bound devices and routed like the group law's (a call lane of its own up to
// LANE_CALL_MAX_UNITS elements, device blocks above).  Not combined: one Fr operation costs nanoseconds on a host core.
constexpr int FR_INVERSE = FR_OPS;
constexpr size_t FR_SHARD_MIN = 4 * 4096;
static int fr_host(int op, const void *a, const void *b, size_t nb, size_t n, void *out) {
    const bool binary = op == FR_ADD || op == FR_SUB || op == FR_MUL;
    if (!n) return GPBC_OK;
    if (!a || !out || (binary && !b)) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    if (binary) TRY(nb_one_or_n(nb, n));
    const bool one = binary && nb == 1;
    HostCall c = HostCall().input(a, GPBC_SCALAR_BYTES);
    if (binary) c.input(b, GPBC_SCALAR_BYTES, one);
    return host_call_sharded(n, FR_SHARD_MIN, c.output(out, GPBC_SCALAR_BYTES), HostRoute{CALL_KINDS, nullptr, 0, LANE_CALL_MAX_UNITS},
                             [=](const DevCols &d, size_t m, hipStream_t st) { return fr_dev(op, d.in[0], d.in[1], one ? 1 : m, m, d.out[0], st); });
}
int gpbc_fr_add_batch(const void *a, const void *b, size_t nb, size_t n, void *o) { return fr_host(FR_ADD, a, b, nb, n, o); }
int gpbc_fr_sub_batch(const void *a, const void *b, size_t nb, size_t n, void *o) { return fr_host(FR_SUB, a, b, nb, n, o); }
int gpbc_fr_mul_batch(const void *a, const void *b, size_t nb, size_t n, void *o) { return fr_host(FR_MUL, a, b, nb, n, o); }
int gpbc_fr_neg_batch(const void *a, size_t n, void *o) { return fr_host(FR_NEG, a, nullptr, n, n, o); }
int gpbc_fr_inverse_batch(const void *a, size_t n, void *o) { return fr_host(FR_INVERSE, a, nullptr, n, n, o); }
int gpbc_fr_from_mont_batch(const void *a, size_t n, void *o) { return fr_host(FR_FROM_MONT, a, nullptr, n, n, o); }
int gpbc_fr_to_mont_batch(const void *a, size_t n, void *o) { return fr_host(FR_TO_MONT, a, nullptr, n, n, o); }
int gpbc_fr_add_batch_dev(const void *a, const void *b, size_t nb, size_t n, void *o, void *st) { return fr_dev(FR_ADD, a, b, nb, n, o, st); }
int gpbc_fr_sub_batch_dev(const void *a, const void *b, size_t nb, size_t n, void *o, void *st) { return fr_dev(FR_SUB, a, b, nb, n, o, st); }
int gpbc_fr_mul_batch_dev(const void *a, const void *b, size_t nb, size_t n, void *o, void *st) { return fr_dev(FR_MUL, a, b, nb, n, o, st); }
int gpbc_fr_neg_batch_dev(const void *a, size_t n, void *o, void *st) { return fr_dev(FR_NEG, a, nullptr, n, n, o, st); }
int gpbc_fr_inverse_batch_dev(const void *a, size_t n, void *o, void *st) { return fr_dev(FR_INVERSE, a, nullptr, n, n, o, st); }
int gpbc_fr_from_mont_batch_dev(const void *a, size_t n, void *o, void *st) { return fr_dev(FR_FROM_MONT, a, nullptr, n, n, o, st); }
int gpbc_fr_to_mont_batch_dev(const void *a, size_t n, void *o, void *st) { return fr_dev(FR_TO_MONT, a, nullptr, n, n, o, st); }

// ------------------------------------------------------------------------------------------------ polynomial entries
static int poly_args(size_t B, size_t k, size_t stride, bool quotients) {
    if (B < 1 || B > (size_t)FR_POLY_MAX_B) return fail(GPBC_ERR_INVALID_ARG, "B must be in 1 .. %d (got %zu)", FR_POLY_MAX_B, B);
    if (quotients && stride < B) return fail(GPBC_ERR_INVALID_ARG, "stride must be at least B (got stride = %zu, B = %zu)", stride, B);
    if (quotients && stride > ((size_t)1 << 24)) return fail(GPBC_ERR_INVALID_ARG, "stride too large (%zu)", stride);
    const size_t blocks = quotients ? (B + BLOCK - 1) / BLOCK : 1;
    return call_limit("polynomials", k, (size_t)0x7fffffff / blocks);
}
int gpbc_fr_poly_from_roots_dev(const void *d_roots, size_t B, size_t k, void *d_coeffs_out, void *stream) {
    TRY(poly_args(B, k, 0, false));
    if (!k) return GPBC_OK;
    if (!d_roots || !d_coeffs_out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    TRY(bind_device());
    return GPBC_LAUNCH(k_fr_poly_from_roots, (unsigned)k, FR_ROOTS_BLOCK, (hipStream_t)stream, (const uint8_t *)d_roots, (uint32_t)B, (uint8_t *)d_coeffs_out);
}
int gpbc_fr_poly_quotients_dev(const void *d_coeffs, const void *d_points, size_t B, size_t k, size_t stride, void *d_q_out, uint8_t *d_ok_out, void *stream) {
    TRY(poly_args(B, k, stride, true));
    if (!k) return GPBC_OK;
    if (!d_coeffs || !d_points || !d_q_out || !d_ok_out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    TRY(bind_device());
    const uint32_t blocks = (uint32_t)((B + BLOCK - 1) / BLOCK);
    if (B <= (size_t)FR_Q_SMALL_B)
        return GPBC_LAUNCH(k_fr_poly_quotients, (unsigned)(k * blocks), BLOCK, (hipStream_t)stream, (const uint8_t *)d_coeffs, (const uint8_t *)d_points, (uint32_t)B, blocks,
                           stride, (uint8_t *)d_q_out, d_ok_out);
    return GPBC_LAUNCH(k_fr_poly_quotients_long, (unsigned)(k * blocks), BLOCK, (hipStream_t)stream, (const uint8_t *)d_coeffs, (const uint8_t *)d_points, (uint32_t)B, blocks,
                       stride, (uint8_t *)d_q_out, d_ok_out);
}
// Host-pointer forms: the unit is a polynomial; a shard needs about 2^16 coefficient steps to pay for its thread and transfers.
static size_t poly_shard_min(size_t B) { return shard_min_units(B * B); }
int gpbc_fr_poly_from_roots(const void *roots, size_t B, size_t k, void *coeffs_out) {
    TRY(poly_args(B, k, 0, false));
    if (!k) return GPBC_OK;
    if (!roots || !coeffs_out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    return host_call_sharded(k, poly_shard_min(B), HostCall().input(roots, B * GPBC_SCALAR_BYTES).output(coeffs_out, (B + 1) * GPBC_SCALAR_BYTES), HostRoute{},
                             [=](const DevCols &d, size_t m, hipStream_t st) { return gpbc_fr_poly_from_roots_dev(d.in[0], B, m, d.out[0], st); });
}
int gpbc_fr_poly_quotients(const void *coeffs, const void *points, size_t B, size_t k, size_t stride, void *q_out, uint8_t *ok_out) {
    TRY(poly_args(B, k, stride, true));
    if (!k) return GPBC_OK;
    if (!coeffs || !points || !q_out || !ok_out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    return host_call_sharded(k, poly_shard_min(B),
                             HostCall().input(coeffs, (B + 1) * GPBC_SCALAR_BYTES).input(points, B * GPBC_SCALAR_BYTES).output(q_out, B * stride * GPBC_SCALAR_BYTES).output(ok_out, B),
                             HostRoute{},
                             [=](const DevCols &d, size_t m, hipStream_t st) { return gpbc_fr_poly_quotients_dev(d.in[0], d.in[1], B, m, stride, d.out[0], d.out[1], st); });
}

// ------------------------------------------------------------------------------------------------ Lagrange basis entries
static int lagrange_args(const void *set, size_t n_set_rows, size_t B, const void *nodes, size_t n_node_rows, size_t m, const void *x, size_t nx, size_t k, const void *out) {
    if (B < 1 || B > (size_t)FR_POLY_MAX_B || m < 1 || m > (size_t)FR_POLY_MAX_B)
        return fail(GPBC_ERR_INVALID_ARG, "B and m must be in 1 .. %d (got B = %zu, m = %zu)", FR_POLY_MAX_B, B, m);
    TRY(call_limit("rows", k));
    if (!k) return GPBC_OK;
    TRY(one_or_k("n_set_rows", n_set_rows, k));
    if (nodes) TRY(one_or_k("n_node_rows", n_node_rows, k));
    if (!nodes && m != B) return fail(GPBC_ERR_INVALID_ARG, "without nodes m must equal B (got m = %zu, B = %zu)", m, B);
    if (x ? nx != 1 && nx != k : nx != 0) return fail(GPBC_ERR_INVALID_ARG, "nx must be 1 or k, or 0 with x == NULL (got nx = %zu, k = %zu)", nx, k);
    if (!set || !out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    const ByteRange r[4] = {{set, n_set_rows * B * GPBC_SCALAR_BYTES}, {nodes, n_node_rows * m * GPBC_SCALAR_BYTES}, {x, nx * GPBC_SCALAR_BYTES}, {out, k * m * GPBC_SCALAR_BYTES}};
    if (outputs_overlap(r, 3, 4)) return fail(GPBC_ERR_INVALID_ARG, "out overlaps an input");
    return GPBC_OK;
}
int gpbc_fr_lagrange_basis_dev(const void *d_set, size_t n_set_rows, size_t B, const void *d_nodes, size_t n_node_rows, size_t m, const void *d_x, size_t nx, size_t k,
                               void *d_out, void *stream) {
    TRY(lagrange_args(d_set, n_set_rows, B, d_nodes, n_node_rows, m, d_x, nx, k, d_out));
    if (!k) return GPBC_OK;
    TRY(bind_device());
    const bool shared_set = n_set_rows == 1 && k > 1;
    const LagrangeGeom g = fr_lagrange_geometry(B, m, shared_set);
    const unsigned grid = (unsigned)fr_lagrange_grid(g, k);
    const size_t set_step = shared_set ? 0 : B * GPBC_SCALAR_BYTES, node_step = d_nodes && n_node_rows == k && k > 1 ? m * GPBC_SCALAR_BYTES : 0,
                 x_step = d_x && nx == k && k > 1 ? GPBC_SCALAR_BYTES : 0;
    const uint8_t *s = (const uint8_t *)d_set, *nd = (const uint8_t *)d_nodes, *xs = (const uint8_t *)d_x;
    if (g.large) return GPBC_LAUNCH(k_fr_lagrange_basis_long, grid, BLOCK, (hipStream_t)stream, s, set_step, nd, node_step, xs, x_step, k, g, (uint8_t *)d_out);
    return GPBC_LAUNCH(k_fr_lagrange_basis, grid, BLOCK, (hipStream_t)stream, s, set_step, nd, node_step, xs, x_step, k, g, (uint8_t *)d_out);
}
// Host-pointer form: the unit is a row; a shard needs about 2^16 factors to pay for its thread and transfers.  A set, a node list or
// an x given once travels whole to every shard.
int gpbc_fr_lagrange_basis(const void *set, size_t n_set_rows, size_t B, const void *nodes, size_t n_node_rows, size_t m, const void *x, size_t nx, size_t k, void *out) {
    TRY(lagrange_args(set, n_set_rows, B, nodes, n_node_rows, m, x, nx, k, out));
    if (!k) return GPBC_OK;
    const bool one_set = n_set_rows == 1, one_nodes = nodes && n_node_rows == 1, one_x = x && nx == 1;
    HostCall c = HostCall().input(set, B * GPBC_SCALAR_BYTES, one_set).input(nodes, m * GPBC_SCALAR_BYTES, one_nodes).input(x, GPBC_SCALAR_BYTES, one_x);
    return host_call_sharded(k, shard_min_units(B * m), c.output(out, m * GPBC_SCALAR_BYTES), HostRoute{},
                             [=](const DevCols &d, size_t rows, hipStream_t st) {
                                 return gpbc_fr_lagrange_basis_dev(d.in[0], one_set ? 1 : rows, B, d.in[1], one_nodes ? 1 : rows, m, d.in[2], d.in[2] ? (one_x ? 1 : rows) : 0, rows, d.out[0], st);
                             });
}

// ------------------------------------------------------------------------------------------------ LSSS weight entries
static int lsss_args(const void *matrix, size_t n_matrices, size_t rows, size_t cols, const void *held, size_t k, const void *w_out, const void *ok_out) {
    if (rows < 1 || rows > (size_t)FR_LSSS_MAX || cols < 1 || cols > (size_t)FR_LSSS_MAX)
        return fail(GPBC_ERR_INVALID_ARG, "rows and cols must be in 1 .. %d (got rows = %zu, cols = %zu)", FR_LSSS_MAX, rows, cols);
    TRY(call_limit("systems", k));
    if (!k) return GPBC_OK;
    TRY(one_or_k("n_matrices", n_matrices, k));
    if (!matrix || !held || !w_out || !ok_out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    const ByteRange r[4] = {{matrix, n_matrices * rows * cols * GPBC_SCALAR_BYTES}, {held, k * rows}, {w_out, k * rows * GPBC_SCALAR_BYTES}, {ok_out, k}};
    if (outputs_overlap(r, 2, 4))
        return fail(GPBC_ERR_INVALID_ARG, "an output overlaps an input or the other output");
    return GPBC_OK;
}
int gpbc_fr_lsss_weights_dev(const void *d_matrix, size_t n_matrices, size_t rows, size_t cols, const uint8_t *d_held, size_t k, void *d_w_out, uint8_t *d_ok_out, void *stream) {
    TRY(lsss_args(d_matrix, n_matrices, rows, cols, d_held, k, d_w_out, d_ok_out));
    if (!k) return GPBC_OK;
    TRY(bind_device());
    const LsssGeom g = fr_lsss_geometry(rows, cols);
    const unsigned grid = (unsigned)fr_lsss_grid(g, k);
    const size_t mat_step = n_matrices == 1 && k > 1 ? 0 : rows * cols * GPBC_SCALAR_BYTES;
    if (g.level == 2) return GPBC_LAUNCH(k_fr_lsss_weights_large, grid, BLOCK, (hipStream_t)stream, (const uint8_t *)d_matrix, mat_step, d_held, k, g, (uint8_t *)d_w_out, d_ok_out);
    if (g.level == 1) return GPBC_LAUNCH(k_fr_lsss_weights_mid, grid, BLOCK, (hipStream_t)stream, (const uint8_t *)d_matrix, mat_step, d_held, k, g, (uint8_t *)d_w_out, d_ok_out);
    return GPBC_LAUNCH(k_fr_lsss_weights, grid, BLOCK, (hipStream_t)stream, (const uint8_t *)d_matrix, mat_step, d_held, k, g, (uint8_t *)d_w_out, d_ok_out);
}
// Host-pointer form: the unit is a system; a shard needs about 2^16 elements to pay for its thread and transfers.  A matrix given
// once travels whole to every shard.
int gpbc_fr_lsss_weights(const void *matrix, size_t n_matrices, size_t rows, size_t cols, const uint8_t *held, size_t k, void *w_out, uint8_t *ok_out) {
    TRY(lsss_args(matrix, n_matrices, rows, cols, held, k, w_out, ok_out));
    if (!k) return GPBC_OK;
    const bool one = n_matrices == 1;
    HostCall c = HostCall().input(matrix, rows * cols * GPBC_SCALAR_BYTES, one).input(held, rows);
    return host_call_sharded(k, shard_min_units(rows * cols), c.output(w_out, rows * GPBC_SCALAR_BYTES).output(ok_out, 1), HostRoute{},
                             [=](const DevCols &d, size_t m, hipStream_t st) { return gpbc_fr_lsss_weights_dev(d.in[0], one ? 1 : m, rows, cols, d.in[1], m, d.out[0], d.out[1], st); });
}

// ------------------------------------------------------------------------------------------------ secret sharing entries (include/gpbc_bn254_share.h)
int gpbc_share_version(void) { return 1; }
static int poly_eval_args(const void *coeffs, size_t n_coeff_rows, size_t d, const void *points, size_t n_point_rows, size_t m, size_t k, const void *out) {
    if (d < 1 || d > (size_t)FR_POLY_MAX_B || m < 1 || m > (size_t)FR_POLY_MAX_B)
        return fail(GPBC_ERR_INVALID_ARG, "d and m must be in 1 .. %d (got d = %zu, m = %zu)", FR_POLY_MAX_B, d, m);
    TRY(call_limit("rows", k));
    if (!k) return GPBC_OK;
    TRY(one_or_k("n_coeff_rows", n_coeff_rows, k));
    TRY(one_or_k("n_point_rows", n_point_rows, k));
    if (!coeffs || !points || !out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    const ByteRange r[3] = {{coeffs, n_coeff_rows * d * GPBC_SCALAR_BYTES}, {points, n_point_rows * m * GPBC_SCALAR_BYTES}, {out, k * m * GPBC_SCALAR_BYTES}};
    if (outputs_overlap(r, 2, 3)) return fail(GPBC_ERR_INVALID_ARG, "out overlaps an input");
    return GPBC_OK;
}
int gpbc_fr_poly_eval_dev(const void *d_coeffs, size_t n_coeff_rows, size_t d, const void *d_points, size_t n_point_rows, size_t m, size_t k, void *d_out, void *stream) {
    TRY(poly_eval_args(d_coeffs, n_coeff_rows, d, d_points, n_point_rows, m, k, d_out));
    if (!k) return GPBC_OK;
    TRY(bind_device());
    const bool shared = n_coeff_rows == 1 && k > 1;
    const PolyEvalGeom g = fr_poly_eval_geometry(d, m, shared);
    const unsigned grid = (unsigned)fr_poly_eval_grid(g, k);
    const size_t coeff_step = shared ? 0 : d * GPBC_SCALAR_BYTES, point_step = n_point_rows == k && k > 1 ? m * GPBC_SCALAR_BYTES : 0;
    if (g.large) return GPBC_LAUNCH(k_fr_poly_eval_long, grid, BLOCK, (hipStream_t)stream, (const uint8_t *)d_coeffs, coeff_step, (const uint8_t *)d_points, point_step, k, g, (uint8_t *)d_out);
    return GPBC_LAUNCH(k_fr_poly_eval, grid, BLOCK, (hipStream_t)stream, (const uint8_t *)d_coeffs, coeff_step, (const uint8_t *)d_points, point_step, k, g, (uint8_t *)d_out);
}
// Host-pointer form: the unit is a row; a shard needs about 2^16 steps to pay for its thread and transfers.  A coefficient row or a point
// row given once travels whole to every shard.
int gpbc_fr_poly_eval(const void *coeffs, size_t n_coeff_rows, size_t d, const void *points, size_t n_point_rows, size_t m, size_t k, void *out) {
    TRY(poly_eval_args(coeffs, n_coeff_rows, d, points, n_point_rows, m, k, out));
    if (!k) return GPBC_OK;
    const bool one_c = n_coeff_rows == 1, one_p = n_point_rows == 1;
    HostCall c = HostCall().input(coeffs, d * GPBC_SCALAR_BYTES, one_c).input(points, m * GPBC_SCALAR_BYTES, one_p);
    return host_call_sharded(k, shard_min_units(d * m), c.output(out, m * GPBC_SCALAR_BYTES), HostRoute{},
                             [=](const DevCols &dc, size_t rows, hipStream_t st) { return gpbc_fr_poly_eval_dev(dc.in[0], one_c ? 1 : rows, d, dc.in[1], one_p ? 1 : rows, m, rows, dc.out[0], st); });
}

// n host tables in one device allocation, each 16-byte aligned, with one copy; at[i]: where table i starts in *block
static hipError_t upload_tables(int n, const void *const *src, const size_t *bytes, void **block, size_t *at) {
    size_t end = 0;
    for (int i = 0; i < n; i++) { at[i] = end; end = (end + bytes[i] + 15) & ~(size_t)15; }
    std::vector<uint8_t> host(end + 16, 0);
    for (int i = 0; i < n; i++)
        if (bytes[i]) memcpy(host.data() + at[i], src[i], bytes[i]);
    *block = nullptr;
    hipError_t e = hipMalloc(block, host.size());
    if (e == hipSuccess) e = hipMemcpy(*block, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess && *block) { (void)hipFree(*block); *block = nullptr; }
    return e;
}
// what both forms of the tree and forest entries refuse, in this order: r[0 .. n_in) are inputs, the rest outputs; a null pointer that
// may be absent has 0 bytes
static int handle_args(const void *h, const char *null_handle, const char *overlaps, size_t k, const ByteRange *r, int n_in, int n) {
    if (!h) return fail(GPBC_ERR_INVALID_ARG, "%s", null_handle);
    TRY(call_limit("items", k));
    if (!k) return GPBC_OK;
    for (int i = 0; i < n; i++)
        if (!r[i].p && r[i].bytes) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    if (outputs_overlap(r, n_in, n)) return fail(GPBC_ERR_INVALID_ARG, "%s", overlaps);
    return GPBC_OK;
}
static int handle_device(int device, const char *what) {
    TRY(bind_device());
    if (current_device() != device) return fail(GPBC_ERR_INVALID_ARG, "%s was created on device %d", what, device);
    return GPBC_OK;
}

// the sharing plan and, behind it, the reconstruction plan of the same node list (recon29.hip.hpp; level_off serves both), in one block
struct gpbc_share_tree {
    int device;
    ShareGeom geom;
    ReconGeom rgeom;
    void *block;
    const ShareUnit *units;
    const uint32_t *level_off;
    const ReconUnit *runits;
    const ReconGate *rgates;
    const uint32_t *rgate_off;
};
int gpbc_share_tree_create(const gpbc_share_node *nodes, size_t n_nodes, gpbc_share_tree **out) {
    static_assert(sizeof(gpbc_share_node) == sizeof(ShareNode), "the public node is the plan's node");
    if (!out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    *out = nullptr;
    SharePlan plan;
    const char *why = fr_share_plan(reinterpret_cast<const ShareNode *>(nodes), n_nodes, plan);
    if (why) return fail(GPBC_ERR_INVALID_ARG, "malformed tree: %s", why);
    ReconPlan rplan;
    why = fr_recon_plan(reinterpret_cast<const ShareNode *>(nodes), n_nodes, rplan);
    if (why) return fail(GPBC_ERR_INVALID_ARG, "malformed tree: %s", why);      // fr_share_plan's reasons: nothing that passed above is refused here
    if (!fr_share_plan_ok(plan)) return fail(GPBC_ERR_INTERNAL, "the sharing plan of a share tree points outside its tables");
    if (!fr_recon_plan_ok(rplan)) return fail(GPBC_ERR_INTERNAL, "the reconstruction plan of a share tree points outside its tables");
    TRY(bind_device());
    const void *src[5] = {plan.units.data(), plan.level_off.data(), rplan.units.data(), rplan.gates.data(), rplan.gate_off.data()};
    const size_t bytes[5] = {plan.units.size() * sizeof(ShareUnit), plan.level_off.size() * sizeof(uint32_t), rplan.units.size() * sizeof(ReconUnit),
                             rplan.gates.size() * sizeof(ReconGate), rplan.gate_off.size() * sizeof(uint32_t)};
    size_t at[5];
    void *block;
    const hipError_t e = upload_tables(5, src, bytes, &block, at);
    if (e != hipSuccess) return fail(GPBC_ERR_HIP, "uploading a share tree failed: %s", hipGetErrorString(e));
    const uint8_t *b = (const uint8_t *)block;
    *out = new gpbc_share_tree{current_device(), fr_share_geometry(plan), fr_recon_geometry(rplan), block, (const ShareUnit *)(b + at[0]), (const uint32_t *)(b + at[1]),
                               (const ReconUnit *)(b + at[2]), (const ReconGate *)(b + at[3]), (const uint32_t *)(b + at[4])};
    return GPBC_OK;
}
int gpbc_share_tree_destroy(gpbc_share_tree *t) {
    if (!t) return GPBC_OK;
    (void)hipSetDevice(t->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(t->block);
    delete t;
    return GPBC_OK;
}
size_t gpbc_share_tree_leaves(const gpbc_share_tree *t) { return t ? t->geom.L : 0; }
size_t gpbc_share_tree_coeffs(const gpbc_share_tree *t) { return t ? t->geom.C : 0; }
static int share_tree_args(const gpbc_share_tree *t, const void *secrets, const void *coeffs, size_t k, const void *out) {
    const size_t S = GPBC_SCALAR_BYTES, L = t ? t->geom.L : 0, C = t ? t->geom.C : 0;
    const ByteRange r[3] = {{secrets, k * S}, {C ? coeffs : nullptr, k * C * S}, {out, k * L * S}};
    return handle_args(t, "null tree handle", "out overlaps an input", k, r, 2, 3);
}
int gpbc_fr_share_tree_dev(const gpbc_share_tree *t, const void *d_secrets, const void *d_coeffs, size_t k, void *d_out, void *stream) {
    TRY(share_tree_args(t, d_secrets, d_coeffs, k, d_out));
    if (!k) return GPBC_OK;
    TRY(handle_device(t->device, "tree"));
    const unsigned grid = (unsigned)fr_share_grid(t->geom, k);
    if (t->geom.large)
        return GPBC_LAUNCH(k_fr_share_tree_large, grid, BLOCK, (hipStream_t)stream, t->units, t->level_off, (const uint8_t *)d_secrets, (const uint8_t *)d_coeffs, k, t->geom, (uint8_t *)d_out);
    return GPBC_LAUNCH(k_fr_share_tree, grid, BLOCK, (hipStream_t)stream, t->units, t->level_off, (const uint8_t *)d_secrets, (const uint8_t *)d_coeffs, k, t->geom, (uint8_t *)d_out);
}
// Host pointers: the shared staging path on the tree's device only (the handle lives there), not combined with other threads' calls.
int gpbc_fr_share_tree(const gpbc_share_tree *t, const void *secrets, const void *coeffs, size_t k, void *out) {
    TRY(share_tree_args(t, secrets, coeffs, k, out));
    if (!k) return GPBC_OK;
    HostCall c = HostCall().input(secrets, GPBC_SCALAR_BYTES);
    if (t->geom.C) c.input(coeffs, t->geom.C * GPBC_SCALAR_BYTES);
    const bool has = t->geom.C != 0;
    return host_call(k, c.output(out, t->geom.L * GPBC_SCALAR_BYTES), HostRoute{CALL_KINDS, nullptr, 0, LANE_CALL_MAX_UNITS},
                     [=](const DevCols &dc, size_t m, hipStream_t st) { return gpbc_fr_share_tree_dev(t, dc.in[0], has ? dc.in[1] : nullptr, m, dc.out[0], st); });
}

// ------------------------------------------------------------------------------------------------ threshold-tree weight entries (include/gpbc_bn254_recon.h)
int gpbc_recon_version(void) { return 1; }
static int tree_weights_args(const gpbc_share_tree *t, const uint8_t *held, size_t k, const void *w_out, const uint8_t *ok_out) {
    const size_t L = t ? t->rgeom.L : 0;
    const ByteRange r[3] = {{held, k * L}, {w_out, k * L * GPBC_SCALAR_BYTES}, {ok_out, k}};
    return handle_args(t, "null tree handle", "an output overlaps an input or the other output", k, r, 1, 3);
}
int gpbc_fr_tree_weights_dev(const gpbc_share_tree *t, const uint8_t *d_held, size_t k, void *d_w_out, uint8_t *d_ok_out, void *stream) {
    TRY(tree_weights_args(t, d_held, k, d_w_out, d_ok_out));
    if (!k) return GPBC_OK;
    TRY(handle_device(t->device, "tree"));
    const unsigned grid = (unsigned)fr_recon_grid(t->rgeom, k);
    if (t->rgeom.large)
        return GPBC_LAUNCH(k_fr_tree_weights_large, grid, BLOCK, (hipStream_t)stream, t->runits, t->level_off, t->rgates, t->rgate_off, d_held, k, t->rgeom, (uint8_t *)d_w_out, d_ok_out);
    return GPBC_LAUNCH(k_fr_tree_weights, grid, BLOCK, (hipStream_t)stream, t->runits, t->level_off, t->rgates, t->rgate_off, d_held, k, t->rgeom, (uint8_t *)d_w_out, d_ok_out);
}
// Host pointers: as gpbc_fr_share_tree, the shared staging path on the tree's device only.
int gpbc_fr_tree_weights(const gpbc_share_tree *t, const uint8_t *held, size_t k, void *w_out, uint8_t *ok_out) {
    TRY(tree_weights_args(t, held, k, w_out, ok_out));
    if (!k) return GPBC_OK;
    const size_t L = t->rgeom.L;
    return host_call(k, HostCall().input(held, L).output(w_out, L * GPBC_SCALAR_BYTES).output(ok_out, 1), HostRoute{CALL_KINDS, nullptr, 0, LANE_CALL_MAX_UNITS},
                     [=](const DevCols &dc, size_t m, hipStream_t st) { return gpbc_fr_tree_weights_dev(t, (const uint8_t *)dc.in[0], m, dc.out[0], (uint8_t *)dc.out[1], st); });
}

// ------------------------------------------------------------------------------------------------ threshold-tree forest entries (include/gpbc_bn254_forest.h)
int gpbc_forest_version(void) { return 1; }
// the block of forest29.hip.hpp in one device allocation, and what the accessors answer from the host
struct gpbc_share_forest {
    int device;
    ForestGeom sgeom, rgeom;
    ForestDev dev;
    void *block;
    std::vector<uint32_t> tree_L, tree_C;
};
int gpbc_share_forest_create(const gpbc_share_node *nodes, const uint32_t *node_off, size_t n_trees, gpbc_share_forest **out) {
    if (!out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    *out = nullptr;
    ForestPlan plan;
    size_t bad = 0;
    const char *why = fr_forest_plan(reinterpret_cast<const ShareNode *>(nodes), node_off, n_trees, plan, &bad);
    if (why && bad < n_trees) return fail(GPBC_ERR_INVALID_ARG, "malformed tree %zu: %s", bad, why);
    if (why) return fail(GPBC_ERR_INVALID_ARG, "malformed forest: %s", why);
    if (!fr_forest_plan_ok(plan)) return fail(GPBC_ERR_INTERNAL, "the plan of a share forest points outside its tables");
    // one block: headers, sharing units, reconstruction units, level offsets, gate offsets, gates
    const size_t bytes[6] = {plan.trees.size() * sizeof(ForestTree), plan.sunits.size() * sizeof(ShareUnit), plan.runits.size() * sizeof(ReconUnit),
                             plan.level_off.size() * sizeof(uint32_t), plan.gate_off.size() * sizeof(uint32_t), plan.gates.size() * sizeof(ReconGate)};
    const void *src[6] = {plan.trees.data(), plan.sunits.data(), plan.runits.data(), plan.level_off.data(), plan.gate_off.data(), plan.gates.data()};
    size_t at[6];
    void *block;
    TRY(bind_device());
    const hipError_t e = upload_tables(6, src, bytes, &block, at);
    if (e != hipSuccess) return fail(GPBC_ERR_HIP, "uploading a share forest failed: %s", hipGetErrorString(e));
    const uint8_t *b = (const uint8_t *)block;
    gpbc_share_forest *h = new gpbc_share_forest{current_device(), fr_forest_share_geometry(plan), fr_forest_recon_geometry(plan),
                                                 ForestDev{(const ForestTree *)(b + at[0]), (const ShareUnit *)(b + at[1]), (const ReconUnit *)(b + at[2]), (const uint32_t *)(b + at[3]),
                                                           (const uint32_t *)(b + at[4]), (const ReconGate *)(b + at[5])},
                                                 block, {}, {}};
    for (const ForestTree &t : plan.trees) { h->tree_L.push_back(t.L); h->tree_C.push_back(t.C); }
    *out = h;
    return GPBC_OK;
}
int gpbc_share_forest_destroy(gpbc_share_forest *f) {
    if (!f) return GPBC_OK;
    (void)hipSetDevice(f->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(f->block);
    delete f;
    return GPBC_OK;
}
size_t gpbc_share_forest_trees(const gpbc_share_forest *f) { return f ? f->sgeom.T : 0; }
size_t gpbc_share_forest_leaves(const gpbc_share_forest *f) { return f ? f->sgeom.Lmax : 0; }
size_t gpbc_share_forest_coeffs(const gpbc_share_forest *f) { return f ? f->sgeom.Cmax : 0; }
size_t gpbc_share_forest_tree_leaves(const gpbc_share_forest *f, size_t t) { return f && t < f->tree_L.size() ? f->tree_L[t] : 0; }
size_t gpbc_share_forest_tree_coeffs(const gpbc_share_forest *f, size_t t) { return f && t < f->tree_C.size() ? f->tree_C[t] : 0; }
static int forest_args(const gpbc_share_forest *f, size_t k, const ByteRange *r, int n_in, int n) {
    return handle_args(f, "null forest handle", "an output overlaps an input or another output", k, r, n_in, n);
}
static int forest_device(const gpbc_share_forest *f) { return handle_device(f->device, "forest"); }
static int share_forest_args(const gpbc_share_forest *f, const void *tree_of, const void *secrets, const void *coeffs, size_t k, const void *out, const void *ok_out) {
    const size_t S = GPBC_SCALAR_BYTES, L = f ? f->sgeom.Lmax : 0, C = f ? f->sgeom.Cmax : 0;
    const ByteRange r[5] = {{tree_of, k * sizeof(uint32_t)}, {secrets, k * S}, {C ? coeffs : nullptr, k * C * S}, {out, k * L * S}, {ok_out, ok_out ? k : 0}};
    return forest_args(f, k, r, 3, 5);
}
int gpbc_fr_share_forest_dev(const gpbc_share_forest *f, const uint32_t *d_tree_of, const void *d_secrets, const void *d_coeffs, size_t k, void *d_out, uint8_t *d_ok_out, void *stream) {
    TRY(share_forest_args(f, d_tree_of, d_secrets, d_coeffs, k, d_out, d_ok_out));
    if (!k) return GPBC_OK;
    TRY(forest_device(f));
    const unsigned grid = (unsigned)fr_forest_grid(f->sgeom, k);
    if (f->sgeom.large)
        return GPBC_LAUNCH(k_fr_share_forest_large, grid, BLOCK, (hipStream_t)stream, f->dev, d_tree_of, (const uint8_t *)d_secrets, (const uint8_t *)d_coeffs, k, f->sgeom, (uint8_t *)d_out, d_ok_out);
    return GPBC_LAUNCH(k_fr_share_forest, grid, BLOCK, (hipStream_t)stream, f->dev, d_tree_of, (const uint8_t *)d_secrets, (const uint8_t *)d_coeffs, k, f->sgeom, (uint8_t *)d_out, d_ok_out);
}
// Host pointers: as gpbc_fr_share_tree, the shared staging path on the forest's device only.
int gpbc_fr_share_forest(const gpbc_share_forest *f, const uint32_t *tree_of, const void *secrets, const void *coeffs, size_t k, void *out, uint8_t *ok_out) {
    TRY(share_forest_args(f, tree_of, secrets, coeffs, k, out, ok_out));
    if (!k) return GPBC_OK;
    TRY(forest_device(f));
    const size_t C = f->sgeom.Cmax;
    HostCall c = HostCall().input(tree_of, sizeof(uint32_t)).input(secrets, GPBC_SCALAR_BYTES);
    if (C) c.input(coeffs, C * GPBC_SCALAR_BYTES);
    return host_call(k, c.output(out, f->sgeom.Lmax * GPBC_SCALAR_BYTES).output(ok_out, 1), HostRoute{CALL_KINDS, nullptr, 0, LANE_CALL_MAX_UNITS},
                     [=](const DevCols &dc, size_t m, hipStream_t st) {
                         return gpbc_fr_share_forest_dev(f, (const uint32_t *)dc.in[0], dc.in[1], C ? dc.in[2] : nullptr, m, dc.out[0], dc.out[1], st);
                     });
}
static int forest_weights_args(const gpbc_share_forest *f, const void *tree_of, const void *held, size_t k, const void *w_out, const void *ok_out) {
    const size_t L = f ? f->rgeom.Lmax : 0;
    const ByteRange r[4] = {{tree_of, k * sizeof(uint32_t)}, {held, k * L}, {w_out, k * L * GPBC_SCALAR_BYTES}, {ok_out, k}};
    return forest_args(f, k, r, 2, 4);
}
int gpbc_fr_forest_weights_dev(const gpbc_share_forest *f, const uint32_t *d_tree_of, const uint8_t *d_held, size_t k, void *d_w_out, uint8_t *d_ok_out, void *stream) {
    TRY(forest_weights_args(f, d_tree_of, d_held, k, d_w_out, d_ok_out));
    if (!k) return GPBC_OK;
    TRY(forest_device(f));
    const unsigned grid = (unsigned)fr_forest_grid(f->rgeom, k);
    if (f->rgeom.large) return GPBC_LAUNCH(k_fr_forest_weights_large, grid, BLOCK, (hipStream_t)stream, f->dev, d_tree_of, d_held, k, f->rgeom, (uint8_t *)d_w_out, d_ok_out);
    return GPBC_LAUNCH(k_fr_forest_weights, grid, BLOCK, (hipStream_t)stream, f->dev, d_tree_of, d_held, k, f->rgeom, (uint8_t *)d_w_out, d_ok_out);
}
int gpbc_fr_forest_weights(const gpbc_share_forest *f, const uint32_t *tree_of, const uint8_t *held, size_t k, void *w_out, uint8_t *ok_out) {
    TRY(forest_weights_args(f, tree_of, held, k, w_out, ok_out));
    if (!k) return GPBC_OK;
    TRY(forest_device(f));
    const size_t L = f->rgeom.Lmax;
    return host_call(k, HostCall().input(tree_of, sizeof(uint32_t)).input(held, L).output(w_out, L * GPBC_SCALAR_BYTES).output(ok_out, 1), HostRoute{CALL_KINDS, nullptr, 0, LANE_CALL_MAX_UNITS},
                     [=](const DevCols &dc, size_t m, hipStream_t st) {
                         return gpbc_fr_forest_weights_dev(f, (const uint32_t *)dc.in[0], (const uint8_t *)dc.in[1], m, dc.out[0], (uint8_t *)dc.out[1], st);
                     });
}

// ------------------------------------------------------------------------------------------------ common attribute entries (include/gpbc_bn254_select.h)
int gpbc_select_version(void) { return 1; }
static int find_common_args(const void *sets, size_t n_sets, size_t m, const void *lists, size_t a, size_t d, size_t k, const void *set_pos_out, const void *list_pos_out,
                            const void *common_out, const void *ok_out) {
    const size_t lim = (size_t)FR_SELECT_MAX;
    if (m < 1 || m > lim || a < 1 || a > lim || d < 1 || d > lim) return fail(GPBC_ERR_INVALID_ARG, "m, a and d must be in 1 .. %d (got m = %zu, a = %zu, d = %zu)", FR_SELECT_MAX, m, a, d);
    TRY(call_limit("items", k));
    if (!k) return GPBC_OK;
    TRY(one_or_k("n_sets", n_sets, k));
    if (!sets || !lists || !set_pos_out || !list_pos_out || !common_out || !ok_out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    const ByteRange r[6] = {{sets, n_sets * m * GPBC_SCALAR_BYTES}, {lists, k * a * GPBC_SCALAR_BYTES}, {set_pos_out, k * d * sizeof(uint32_t)}, {list_pos_out, k * d * sizeof(uint32_t)},
                            {common_out, k * d * GPBC_SCALAR_BYTES}, {ok_out, k}};
    if (outputs_overlap(r, 2, 6)) return fail(GPBC_ERR_INVALID_ARG, "an output overlaps an input or another output");
    return GPBC_OK;
}
int gpbc_fr_find_common_dev(const void *d_sets, size_t n_sets, size_t m, const void *d_lists, size_t a, size_t d, size_t k, uint32_t *d_set_pos_out, uint32_t *d_list_pos_out,
                            void *d_common_out, uint8_t *d_ok_out, void *stream) {
    TRY(find_common_args(d_sets, n_sets, m, d_lists, a, d, k, d_set_pos_out, d_list_pos_out, d_common_out, d_ok_out));
    if (!k) return GPBC_OK;
    TRY(bind_device());
    const SelectGeom g = fr_select_geometry(m, a, d, n_sets == 1);
    const SelectOut o{(uint8_t *)d_set_pos_out, (uint8_t *)d_list_pos_out, (uint8_t *)d_common_out, d_ok_out, d * sizeof(uint32_t), d * GPBC_SCALAR_BYTES};
    const unsigned grid = (unsigned)fr_select_grid(g, k);
    if (g.large) return GPBC_LAUNCH(k_fr_find_common_large, grid, BLOCK, (hipStream_t)stream, (const uint8_t *)d_sets, (const uint8_t *)d_lists, k, g, o);
    return GPBC_LAUNCH(k_fr_find_common, grid, BLOCK, (hipStream_t)stream, (const uint8_t *)d_sets, (const uint8_t *)d_lists, k, g, o);
}
// Host-pointer form: the unit is an item; a shard needs about 2^16 comparisons to pay for its thread and transfers.  A set given once
// travels whole to every shard; the four outputs are the staging path's four output columns.
int gpbc_fr_find_common(const void *sets, size_t n_sets, size_t m, const void *lists, size_t a, size_t d, size_t k, uint32_t *set_pos_out, uint32_t *list_pos_out, void *common_out,
                        uint8_t *ok_out) {
    TRY(find_common_args(sets, n_sets, m, lists, a, d, k, set_pos_out, list_pos_out, common_out, ok_out));
    if (!k) return GPBC_OK;
    const bool one = n_sets == 1;
    HostCall c = HostCall().input(sets, m * GPBC_SCALAR_BYTES, one).input(lists, a * GPBC_SCALAR_BYTES);
    c.output(set_pos_out, d * sizeof(uint32_t)).output(list_pos_out, d * sizeof(uint32_t)).output(common_out, d * GPBC_SCALAR_BYTES).output(ok_out, 1);
    return host_call_sharded(k, shard_min_units(m * a), c, HostRoute{}, [=](const DevCols &dc, size_t n, hipStream_t st) {
        return gpbc_fr_find_common_dev(dc.in[0], one ? 1 : n, m, dc.in[1], a, d, n, (uint32_t *)dc.out[0], (uint32_t *)dc.out[1], dc.out[2], dc.out[3], st);
    });
}

// ------------------------------------------------------------------------------------------------ LSSS share entries (include/gpbc_bn254_indexed.h)
static int lsss_shares_args(const void *matrix, size_t n_matrices, size_t rows, size_t cols, const void *vectors, size_t k, const void *out) {
    if (rows < 1 || rows > (size_t)FR_LSSS_MAX || cols < 1 || cols > (size_t)FR_LSSS_MAX)
        return fail(GPBC_ERR_INVALID_ARG, "rows and cols must be in 1 .. %d (got rows = %zu, cols = %zu)", FR_LSSS_MAX, rows, cols);
    TRY(call_limit("vectors", k));
    if (!k) return GPBC_OK;
    TRY(one_or_k("n_matrices", n_matrices, k));
    if (!matrix || !vectors || !out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    const ByteRange r[3] = {{matrix, n_matrices * rows * cols * GPBC_SCALAR_BYTES}, {vectors, k * cols * GPBC_SCALAR_BYTES}, {out, k * rows * GPBC_SCALAR_BYTES}};
    if (outputs_overlap(r, 2, 3)) return fail(GPBC_ERR_INVALID_ARG, "out overlaps an input");
    return GPBC_OK;
}
int gpbc_fr_lsss_shares_dev(const void *d_matrix, size_t n_matrices, size_t rows, size_t cols, const void *d_vectors, size_t k, void *d_out, void *stream) {
    TRY(lsss_shares_args(d_matrix, n_matrices, rows, cols, d_vectors, k, d_out));
    if (!k) return GPBC_OK;
    TRY(bind_device());
    const bool shared = n_matrices == 1 && k > 1;
    const LsssSharesGeom g = fr_lsss_shares_geometry(rows, cols, shared);
    const size_t mat_step = shared ? 0 : rows * cols * GPBC_SCALAR_BYTES;
    return GPBC_LAUNCH(k_fr_lsss_shares, (unsigned)fr_lsss_shares_grid(g, k), BLOCK, (hipStream_t)stream, (const uint8_t *)d_matrix, mat_step, (const uint8_t *)d_vectors, k, g, (uint8_t *)d_out);
}
// Host-pointer form: the unit is a vector; a shard needs about 2^16 products to pay for its thread and transfers.  A matrix given once
// travels whole to every shard.
int gpbc_fr_lsss_shares(const void *matrix, size_t n_matrices, size_t rows, size_t cols, const void *vectors, size_t k, void *out) {
    TRY(lsss_shares_args(matrix, n_matrices, rows, cols, vectors, k, out));
    if (!k) return GPBC_OK;
    const bool one = n_matrices == 1;
    HostCall c = HostCall().input(matrix, rows * cols * GPBC_SCALAR_BYTES, one).input(vectors, cols * GPBC_SCALAR_BYTES);
    return host_call_sharded(k, shard_min_units(rows * cols), c.output(out, rows * GPBC_SCALAR_BYTES), HostRoute{},
                             [=](const DevCols &d, size_t m, hipStream_t st) { return gpbc_fr_lsss_shares_dev(d.in[0], one ? 1 : m, rows, cols, d.in[1], m, d.out[0], st); });
}

// ------------------------------------------------------------------------------------------------ formula entries (include/gpbc_bn254_formula.h)
int gpbc_formula_version(void) { return 1; }
static int formula_sizes(size_t n_nodes, size_t rows, size_t cols, size_t k) {
    if (n_nodes < 1 || n_nodes > (size_t)FORMULA_MAX_NODES) return fail(GPBC_ERR_INVALID_ARG, "n_nodes must be in 1 .. %d (got %zu)", FORMULA_MAX_NODES, n_nodes);
    if (rows < 1 || rows > (size_t)FORMULA_MAX || cols < 1 || cols > (size_t)FORMULA_MAX)
        return fail(GPBC_ERR_INVALID_ARG, "rows and cols must be in 1 .. %d (got rows = %zu, cols = %zu)", FORMULA_MAX, rows, cols);
    return call_limit("items", k);
}
static int from_formula_args(const void *nodes, size_t n_nodes, size_t k, size_t rows, size_t cols, const void *matrix_out, const void *rho_out, const void *dims_out, const void *ok_out) {
    TRY(formula_sizes(n_nodes, rows, cols, k));
    if (!k) return GPBC_OK;
    if (!nodes || !matrix_out || !rho_out || !ok_out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    const ByteRange r[5] = {{nodes, k * n_nodes * sizeof(int64_t)}, {matrix_out, k * rows * cols * GPBC_SCALAR_BYTES}, {rho_out, k * rows * sizeof(int64_t)}, {ok_out, k},
                            {dims_out, k * 2 * sizeof(uint32_t)}};
    if (outputs_overlap(r, 1, 5)) return fail(GPBC_ERR_INVALID_ARG, "an output overlaps the input or another output");
    return GPBC_OK;
}
// The kernel stores a matrix 128 bits at a time when its address and pitch allow it.  From the host form they always do: every staging route
// starts a column at a 256-byte aligned device address (a lane's pinned block, a device block) and the matrix pitch, rows x cols x 32 bytes,
// is a multiple of 32 — so is the step of a pipelined chunk.
int gpbc_fr_lsss_from_formula_dev(const int64_t *d_nodes, size_t n_nodes, size_t k, size_t rows, size_t cols, void *d_matrix_out, int64_t *d_rho_out, uint32_t *d_dims_out,
                                  uint8_t *d_ok_out, void *stream) {
    TRY(from_formula_args(d_nodes, n_nodes, k, rows, cols, d_matrix_out, d_rho_out, d_dims_out, d_ok_out));
    if (!k) return GPBC_OK;
    TRY(bind_device());
    const FormulaOut o{(uint8_t *)d_matrix_out, (uint8_t *)d_rho_out, (uint8_t *)d_dims_out, d_ok_out, rows * cols * GPBC_SCALAR_BYTES, rows * sizeof(int64_t), 2 * sizeof(uint32_t)};
    const FormulaGeom g = formula_build_geometry(n_nodes, rows, cols, (((uintptr_t)o.matrix | o.mat_step) & 15) == 0);
    return GPBC_LAUNCH(k_fr_lsss_from_formula, (unsigned)formula_grid(g, k), BLOCK, (hipStream_t)stream, d_nodes, k, g, o);
}
// Host-pointer form: the shared staging path on the current device, the four outputs as its four output columns (dims_out == NULL: that
// column is not wanted, and the device form is told so).
int gpbc_fr_lsss_from_formula(const int64_t *nodes, size_t n_nodes, size_t k, size_t rows, size_t cols, void *matrix_out, int64_t *rho_out, uint32_t *dims_out, uint8_t *ok_out) {
    TRY(from_formula_args(nodes, n_nodes, k, rows, cols, matrix_out, rho_out, dims_out, ok_out));
    if (!k) return GPBC_OK;
    HostCall c = HostCall().input(nodes, n_nodes * sizeof(int64_t));
    c.output(matrix_out, rows * cols * GPBC_SCALAR_BYTES).output(rho_out, rows * sizeof(int64_t)).output(dims_out, 2 * sizeof(uint32_t)).output(ok_out, 1);
    return host_call(k, c, HostRoute{}, [=](const DevCols &dc, size_t n, hipStream_t st) {
        return gpbc_fr_lsss_from_formula_dev((const int64_t *)dc.in[0], n_nodes, n, rows, cols, dc.out[0], (int64_t *)dc.out[1], (uint32_t *)dc.out[2], dc.out[3], st);
    });
}
static int formula_select_args(const void *nodes, size_t n_formulas, size_t n_nodes, const void *held, size_t k, size_t rows, const void *chosen_out, const void *ok_out) {
    TRY(formula_sizes(n_nodes, rows, 1, k));
    if (!k) return GPBC_OK;
    TRY(one_or_k("n_formulas", n_formulas, k));
    if (!nodes || !held || !chosen_out || !ok_out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    const ByteRange r[4] = {{nodes, n_formulas * n_nodes * sizeof(int64_t)}, {held, k * rows}, {chosen_out, k * rows}, {ok_out, k}};
    if (outputs_overlap(r, 2, 4))
        return fail(GPBC_ERR_INVALID_ARG, "an output overlaps an input or the other output");
    return GPBC_OK;
}
int gpbc_formula_select_dev(const int64_t *d_nodes, size_t n_formulas, size_t n_nodes, const uint8_t *d_held, size_t k, size_t rows, uint8_t *d_chosen_out, uint8_t *d_ok_out,
                            void *stream) {
    TRY(formula_select_args(d_nodes, n_formulas, n_nodes, d_held, k, rows, d_chosen_out, d_ok_out));
    if (!k) return GPBC_OK;
    TRY(bind_device());
    const FormulaGeom g = formula_select_geometry(n_nodes, rows, n_formulas == 1 && k > 1);
    return GPBC_LAUNCH(k_formula_select, (unsigned)formula_grid(g, k), BLOCK, (hipStream_t)stream, d_nodes, d_held, k, g, d_chosen_out, d_ok_out);
}
// Host-pointer form: the shared staging path on the current device; one formula travels once.
int gpbc_formula_select(const int64_t *nodes, size_t n_formulas, size_t n_nodes, const uint8_t *held, size_t k, size_t rows, uint8_t *chosen_out, uint8_t *ok_out) {
    TRY(formula_select_args(nodes, n_formulas, n_nodes, held, k, rows, chosen_out, ok_out));
    if (!k) return GPBC_OK;
    const bool one = n_formulas == 1;
    return host_call(k, HostCall().input(nodes, n_nodes * sizeof(int64_t), one).input(held, rows).output(chosen_out, rows).output(ok_out, 1), HostRoute{},
                     [=](const DevCols &dc, size_t n, hipStream_t st) {
                         return gpbc_formula_select_dev((const int64_t *)dc.in[0], one ? 1 : n, n_nodes, dc.in[1], n, rows, dc.out[0], dc.out[1], st);
                     });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ segmented inner products (include/gpbc_bn254_verify.h)
// L lanes per piece, 64 / L pieces per wavefront (= workgroup) (segred_piece: clamped table, uniform folds, a shared list never overrun):
// the L lanes stride the piece's elements, EVERY lane of the wavefront runs the wavefront's trip count — a piece slot past the last piece
// is an empty piece, no lane leaves early — and log2(L) butterfly steps fold the L partial sums (csrc/frdot29.hip.hpp).
__global__ void __launch_bounds__(BLOCK, FR_DOT_WAVES_PER_SIMD) k_fr_dot_segments(SegRedArgs g, uint32_t L, int wide_x, int wide_k) {
    const uint32_t lane = threadIdx.x % L;
    size_t lo = 0, a = 0, b = 0, P = 0;
    const bool have = segred_piece(g, (size_t)blockIdx.x * (FR_DOT_WAVE / L) + threadIdx.x / L, lo, a, b, P);
    if (!have) lo = a = b = 0;
    unsigned long long rounds = fr_dot_rounds(b - a, L);
    for (uint32_t off = FR_DOT_WAVE / 2; off >= L; off >>= 1) {           // the largest of the wavefront's pieces
        const unsigned long long o = __shfl_xor(rounds, (int)off, FR_DOT_WAVE);
        rounds = o > rounds ? o : rounds;
    }
    Fr v = fr_dot_lane(g.x, g.k, g.k_shared ? lo : 0, a, b, lane, L, (size_t)rounds, wide_x != 0, wide_k != 0);
    for (uint32_t off = L / 2; off >= 1; off >>= 1) {
        Fr o;
#pragma unroll
        for (int i = 0; i < NL; i++) o.l.v[i] = __shfl_xor(v.l.v[i], (int)off, FR_DOT_WAVE);
        v = fr_dot_fold(v, o);
    }
    if (have && lane == 0) fr_dot_store(g.out + P * GPBC_SCALAR_BYTES, v);
}
static int fr_dot_launch(const SegRedArgs &g, int32_t *, hipStream_t st) {
    const uint32_t L = fr_dot_lanes(g), per_wave = FR_DOT_WAVE / L;
    return GPBC_LAUNCH(k_fr_dot_segments, (unsigned)((g.n_pieces + per_wave - 1) / per_wave), BLOCK, st, g, L, (int)(((uintptr_t)g.x & 15) == 0), (int)(((uintptr_t)g.k & 15) == 0));
}
// no tables; the piece values are read 128 bits at a time; the host form is one call
static const SegRedOp FR_DOT_OP{FR_DOT_SHAPE, GPBC_SCALAR_BYTES, 0, 16, "elements", "second operands", "second operand", "a", "gpbc_fr_dot_segments_workspace_bytes", fr_dot_launch, false};

extern "C" {

int gpbc_verify_version(void) { return 1; }
size_t gpbc_fr_dot_segments_workspace_bytes(size_t n, size_t n_seg) { return segred_workspace_bytes(FR_DOT_OP, n, n_seg); }
int gpbc_fr_dot_segments_dev(const void *d_a, const void *d_b, size_t nb, const uint64_t *d_seg_off, size_t n, size_t n_seg, void *d_out, void *d_workspace,
                             size_t workspace_bytes, void *stream) {
    if (!n_seg) return GPBC_OK;
    return segred_dev(FR_DOT_OP, d_a, d_b, nb, d_seg_off, n, n_seg, d_out, d_workspace, workspace_bytes, stream);
}
int gpbc_fr_dot_segments(const void *a, const void *b, size_t nb, const uint64_t *seg_off, size_t n_seg, void *out) {
    if (!n_seg) return GPBC_OK;
    return segred_host(FR_DOT_OP, a, b, nb, seg_off, n_seg, out);
}

}  // extern "C"
