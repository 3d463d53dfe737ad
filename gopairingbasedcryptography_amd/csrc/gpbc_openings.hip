// libgpbc_bn254.so, the fourteenth unit (_build.OPENINGS_SOURCES): batch polynomials over segments of any length and opening proofs over the
// fixed-base window tables with the quotient's coefficients made in the lane that adds their terms (csrc/openings29.hip.hpp), with the C-ABI
// entries of include/gpbc_bn254_openings.h.  gfx950 only.
// A unit of its own, and not beside fb_msm_lane in gpbc_curve.hip or the polynomial kernels in gpbc_fr.hip, for the reason at the head of
// csrc/gpbc_gtfixed.hip: every older unit stays the parent's source and compiles to the parent's code.  The price: the handle's struct and
// fb_shape's rule are restated here (gpbc_fixed_base below, opn_shape), and the point sums of the chunks go through point_sum_strided_dev.
#include "gpbc_common.hpp"
#include "openings29.hip.hpp"
#include "../../include/gpbc_bn254_openings.h"

// the handle of gpbc_g1/g2_fixed_base_create as gpbc_curve.hip defines it, member for member; the table is that unit's too:
// entry ((b * 32 + w) * 255 + d - 1) = [d * 2^(8w)] base_b
struct gpbc_fixed_base { int device; int is_g2; size_t nbase; int32_t *table; uint8_t *base_inf; };

__device__ __forceinline__ Fr opn_lds_get(const int32_t *p) {
    Fr x;
#pragma unroll
    for (int i = 0; i < NL; i++) x.l.v[i] = p[i];
    return x;
}
__device__ __forceinline__ void opn_lds_put(int32_t *p, const Fr &x) {
#pragma unroll
    for (int i = 0; i < NL; i++) p[i] = x.l.v[i];
}

// prod_{i in segment j} (X - roots[i]): k_fr_poly_from_roots (gpbc_fr.hip) with the segment's own length for B and rows of `stride`
// scalars, zero behind the m + 1 coefficients.  One workgroup per segment; the same steps in the same order, so a full segment gives the
// same bytes.
constexpr int OPN_ROOTS_BLOCK = 256, OPN_ROOTS_OWN = (FR_POLY_MAX_B + OPN_ROOTS_BLOCK) / OPN_ROOTS_BLOCK;
__global__ void __launch_bounds__(OPN_ROOTS_BLOCK) k_fr_poly_from_roots_segments(const uint8_t *__restrict__ roots, const uint64_t *__restrict__ seg_off, size_t stride,
                                                                                 uint8_t *__restrict__ coeffs_out) {
    __shared__ int32_t cs[(FR_POLY_MAX_B + 1) * NL];
    __shared__ int32_t rs[64 * NL];
    const uint32_t tid = threadIdx.x;
    const uint64_t lo = seg_off[blockIdx.x];
    const uint32_t B = (uint32_t)(seg_off[blockIdx.x + 1] - lo);             // <= FR_POLY_MAX_B, < stride: checked by the entry
    const uint8_t *rt = roots + lo * 32;
    uint8_t *out = coeffs_out + (size_t)blockIdx.x * stride * 32;
    for (uint32_t i = tid; i <= B; i += OPN_ROOTS_BLOCK) opn_lds_put(cs + i * NL, i ? fr_zero() : fr_plain_one());
    __syncthreads();
    for (uint32_t s = 0; s < B; s++) {
        if ((s & 63) == 0) {
            if (tid < 64 && s + tid < B) opn_lds_put(rs + tid * NL, fr_poly_neg_root(rt + 32 * (size_t)(s + tid)));
            __syncthreads();
        }
        const Fr nr = opn_lds_get(rs + (s & 63) * NL);
        Fr nw[OPN_ROOTS_OWN];
#pragma unroll
        for (int m = 0; m < OPN_ROOTS_OWN; m++) {
            const uint32_t i = tid + m * OPN_ROOTS_BLOCK;
            if (i <= s + 1) nw[m] = fr_poly_root_step(i ? opn_lds_get(cs + (i - 1) * NL) : fr_zero(), opn_lds_get(cs + i * NL), nr);
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < OPN_ROOTS_OWN; m++) {
            const uint32_t i = tid + m * OPN_ROOTS_BLOCK;
            if (i <= s + 1) opn_lds_put(cs + i * NL, nw[m]);
        }
        __syncthreads();
    }
    for (uint32_t i = tid; i <= B; i += OPN_ROOTS_BLOCK) fr_poly_store(out + 32 * (size_t)i, opn_lds_get(cs + i * NL));
    uint32_t *pad = reinterpret_cast<uint32_t *>(out);
    for (size_t w = (size_t)(B + 1) * 8 + tid; w < stride * 8; w += OPN_ROOTS_BLOCK) pad[w] = 0;
}

// A workgroup is one wave: (block of up to 64 identities of ONE segment, chunk of C bases); the workgroups run chunk-major, so the partial
// sums are partial[chunk * n + identity], the order the strided point sum folds.  f waits in LDS in canonical limbs (every lane reads the
// same address: a broadcast).  A wave whose chunk lies past its segment's degree stages nothing and writes the point at infinity.
// Two instances as for the quotients: LDS for segments up to 256 (9 KB) and up to 1024 (36 KB).
template <class F, uint32_t MAXM> __device__ __forceinline__ void fb_openings_kernel(const int32_t *table, const uint8_t *base_inf, size_t nbase, const uint8_t *coeffs, const uint8_t *ids,
                                                                                     const OpnBlock *blocks, uint32_t n_blocks, size_t n, uint32_t C, uint8_t *partial, uint8_t *ok) {
    __shared__ int32_t cs[(MAXM + 1) * NL];
    const uint32_t lane = threadIdx.x, chunk = blockIdx.x / n_blocks;
    const OpnBlock b = blocks[blockIdx.x % n_blocks];
    const uint32_t c_lo = chunk * C, c_hi = (size_t)c_lo + C < nbase ? c_lo + C : (uint32_t)nbase;
    if (c_lo < b.m) {                                                        // uniform over the workgroup
        const uint8_t *f = coeffs + (size_t)b.seg * nbase * 32;
        for (uint32_t i = lane; i <= b.m; i += BLOCK) opn_lds_put(cs + i * NL, fr_poly_coeff_in(f + 32 * (size_t)i));
        __syncthreads();
    }
    if (lane >= b.rows) return;
    const size_t i = (size_t)b.id0 + lane;
    constexpr size_t PT = sizeof(F) == sizeof(Fe) ? GPBC_G1_BYTES : GPBC_G2_BYTES;
    fb_openings_lane<F>(table, base_inf, [&](uint32_t c) { return opn_lds_get(cs + c * NL); }, b.m, ids + 32 * i, c_lo, c_hi, C >= nbase, partial + ((size_t)chunk * n + i) * PT,
                        ok ? ok + i : nullptr, [](uint8_t *p, const AffP<F> &a) { if constexpr (sizeof(F) == sizeof(Fe)) g1_store_aff(p, a); else g2_store_aff(p, a); });
}
#define OPN_ARGS const int32_t *__restrict__ table, const uint8_t *__restrict__ base_inf, size_t nbase, const uint8_t *__restrict__ coeffs, const uint8_t *__restrict__ ids, \
                 const OpnBlock *__restrict__ blocks, uint32_t n_blocks, size_t n, uint32_t C, uint8_t *__restrict__ partial, uint8_t *__restrict__ ok
#define OPN_PASS table, base_inf, nbase, coeffs, ids, blocks, n_blocks, n, C, partial, ok
GPBC_KERNEL_G1 k_g1_fb_openings(OPN_ARGS) { fb_openings_kernel<Fe, OPN_SMALL_M>(OPN_PASS); }
GPBC_KERNEL k_g2_fb_openings(OPN_ARGS) { fb_openings_kernel<F2, OPN_SMALL_M>(OPN_PASS); }
// the long instances: 36 KB of LDS per wave leave one wave per SIMD whatever the registers, so no occupancy is asked for
__global__ void __launch_bounds__(BLOCK) k_g1_fb_openings_long(OPN_ARGS) { fb_openings_kernel<Fe, OPN_MAX_M>(OPN_PASS); }
__global__ void __launch_bounds__(BLOCK) k_g2_fb_openings_long(OPN_ARGS) { fb_openings_kernel<F2, OPN_MAX_M>(OPN_PASS); }

// after the chunks have been added: the rows whose identity is not a root exactly once become all zero
__global__ void __launch_bounds__(BLOCK) k_fb_openings_mask(const uint8_t *__restrict__ ok, size_t n, uint32_t words, uint32_t *__restrict__ out) {
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n * words) return;
    if (!ok[t / words]) out[t] = 0;
}

// ---- small host tables on their way to the device without a synchronisation: a ring of pinned buffers, each with the event of the copy
// that last read it.  A slot is reused only after that copy has run (eight calls later it has, as a rule: the wait is a formality).
namespace {
struct TableSlot { void *pin = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; int device = -1; };
constexpr int TABLE_SLOTS = 8;
std::mutex g_table_mu;
TableSlot g_table_ring[TABLE_SLOTS];
unsigned g_table_next = 0;
int upload_table_async(const void *src, size_t bytes, void *d_dst, hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_table_mu);
    TableSlot &s = g_table_ring[g_table_next++ % TABLE_SLOTS];
    if (s.ev) HIP_TRY(hipEventSynchronize(s.ev));
    if (s.ev && s.device != current_device()) { (void)hipEventDestroy(s.ev); s.ev = nullptr; }
    if (s.cap < bytes) {
        if (s.pin) (void)hipHostFree(s.pin);
        s.pin = nullptr; s.cap = 0;
        const size_t cap = bytes < 4096 ? 4096 : (bytes + 4095) & ~(size_t)4095;
        HIP_TRY(hipHostMalloc(&s.pin, cap, hipHostMallocPortable));
        s.cap = cap;
    }
    if (!s.ev) { HIP_TRY(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming)); s.device = current_device(); }
    memcpy(s.pin, src, bytes);
    HIP_TRY(hipMemcpyAsync(d_dst, s.pin, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s.ev, st));
    return GPBC_OK;
}
// the segment table and what it implies: *n = identities, *m_max = the longest segment; limit = the longest segment allowed
int opn_segments(const uint64_t *seg_off, size_t k, size_t limit, const char *limit_text, size_t *n, size_t *m_max) {
    TRY(call_limit("segments", k, 0x7fffffff));
    TRY(check_segment_table(seg_off, k, n));
    *m_max = 0;
    for (size_t j = 0; j < k; j++) {
        const uint64_t m = seg_off[j + 1] - seg_off[j];
        if (m > limit) return fail(GPBC_ERR_INVALID_ARG, "segment %zu holds %llu elements, %s allows %zu", j, (unsigned long long)m, limit_text, limit);
        if (m > *m_max) *m_max = (size_t)m;
    }
    return GPBC_OK;
}
int roots_segments_args(const void *roots, const uint64_t *seg_off, size_t k, size_t stride, const void *coeffs_out, size_t *n) {
    if (stride < 1 || stride > ((size_t)1 << 24)) return fail(GPBC_ERR_INVALID_ARG, "stride must be in 1 .. 2^24 (got %zu)", stride);
    size_t m_max = 0;
    const size_t limit = stride - 1 < (size_t)FR_POLY_MAX_B ? stride - 1 : (size_t)FR_POLY_MAX_B;
    TRY(opn_segments(seg_off, k, limit, stride - 1 < (size_t)FR_POLY_MAX_B ? "stride - 1" : "FR_POLY_MAX_B", n, &m_max));
    if ((*n && !roots) || !coeffs_out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    if (ranges_overlap(coeffs_out, k * stride * GPBC_SCALAR_BYTES, roots, *n * GPBC_SCALAR_BYTES)) return fail(GPBC_ERR_INVALID_ARG, "coeffs_out overlaps the roots");
    return GPBC_OK;
}
int openings_args(const gpbc_fixed_base *h, const void *coeffs, const void *ids, const uint64_t *seg_off, size_t k, const void *out, const uint8_t *ok_out, size_t *n, size_t *m_max) {
    if (!h) return fail(GPBC_ERR_INVALID_ARG, "null table handle");
    TRY(opn_segments(seg_off, k, h->nbase - 1 < (size_t)FR_POLY_MAX_B ? h->nbase - 1 : (size_t)FR_POLY_MAX_B, h->nbase - 1 < (size_t)FR_POLY_MAX_B ? "nbase - 1" : "FR_POLY_MAX_B", n, m_max));
    TRY(call_limit("identities", *n, 0x7fffffff));
    if (!*n) return GPBC_OK;
    if (!coeffs || !ids || !out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    const ByteRange r[4] = {{coeffs, k * h->nbase * GPBC_SCALAR_BYTES}, {ids, *n * GPBC_SCALAR_BYTES}, {out, *n * (h->is_g2 ? GPBC_G2_BYTES : GPBC_G1_BYTES)}, {ok_out, *n}};
    if (outputs_overlap(r, 2, 4))
        return fail(GPBC_ERR_INVALID_ARG, "an output overlaps an input or the other output");
    return GPBC_OK;
}
// partial sums of every level of the fan-in-16 reduction over the chunks, then the n flags the mask reads
size_t openings_partial_bytes(const gpbc_fixed_base *h, size_t n) {
    size_t C, n_chunks, total = 0;
    opn_shape(h->nbase, n, &C, &n_chunks);
    for (size_t c = n_chunks; c > 1; c = (c + 15) / 16) total += c * n;
    return Scratch::padded(total * (h->is_g2 ? GPBC_G2_BYTES : GPBC_G1_BYTES));
}
}  // namespace

extern "C" {

int gpbc_openings_version(void) { return 1; }

int gpbc_fr_poly_from_roots_segments_dev(const void *d_roots, const uint64_t *seg_off, size_t k, size_t stride, void *d_coeffs_out, void *stream) {
    if (!k) return GPBC_OK;
    size_t n = 0;
    TRY(roots_segments_args(d_roots, seg_off, k, stride, d_coeffs_out, &n));
    TRY(bind_device());
    hipStream_t st = (hipStream_t)stream;
    const size_t seg_bytes = (k + 1) * sizeof(uint64_t);
    Scratch tmp;
    TRY(tmp.open(st, 0, Scratch::padded(seg_bytes)));
    uint64_t *d_seg = tmp.take<uint64_t>(seg_bytes);
    TRY(upload_table_async(seg_off, seg_bytes, d_seg, st));
    return GPBC_LAUNCH(k_fr_poly_from_roots_segments, (unsigned)k, OPN_ROOTS_BLOCK, st, (const uint8_t *)d_roots, d_seg, stride, (uint8_t *)d_coeffs_out);
}
// Host pointers: the unit of the staging path is a segment (a row of coeffs_out); the roots travel as one column.
int gpbc_fr_poly_from_roots_segments(const void *roots, const uint64_t *seg_off, size_t k, size_t stride, void *coeffs_out) {
    if (!k) return GPBC_OK;
    size_t n = 0;
    TRY(roots_segments_args(roots, seg_off, k, stride, coeffs_out, &n));
    return host_call(k, HostCall().input(roots, n * GPBC_SCALAR_BYTES, true).output(coeffs_out, stride * GPBC_SCALAR_BYTES), HostRoute{},
                     [=](const DevCols &d, size_t, hipStream_t st) { return gpbc_fr_poly_from_roots_segments_dev(d.in[0], seg_off, k, stride, d.out[0], st); });
}

size_t gpbc_fixed_base_openings_workspace_bytes(const gpbc_fixed_base *h, size_t n) {
    if (!h || !n) return 0;
    const size_t partial = openings_partial_bytes(h, n);
    return partial ? partial + Scratch::padded(n) : 0;
}
int gpbc_fixed_base_openings_dev(const gpbc_fixed_base *h, const void *d_coeffs, const void *d_ids, const uint64_t *seg_off, size_t k, void *d_out, uint8_t *d_ok_out, void *d_workspace,
                                 size_t workspace_bytes, void *stream) {
    if (!k) return h ? GPBC_OK : fail(GPBC_ERR_INVALID_ARG, "null table handle");
    size_t n = 0, m_max = 0;
    TRY(openings_args(h, d_coeffs, d_ids, seg_off, k, d_out, d_ok_out, &n, &m_max));
    if (!n) return GPBC_OK;
    size_t C, n_chunks;
    opn_shape(h->nbase, n, &C, &n_chunks);
    const size_t n_blocks = opn_blocks(seg_off, k, nullptr);
    if (n_blocks * n_chunks > (size_t)0x7fffffff) return fail(GPBC_ERR_INVALID_ARG, "too many identities for one call (%zu)", n);
    const size_t need = gpbc_fixed_base_openings_workspace_bytes(h, n);
    if (need && (!d_workspace || workspace_bytes < need)) return fail(GPBC_ERR_WORKSPACE, "workspace too small");
    TRY(bind_device());
    if (current_device() != h->device) return fail(GPBC_ERR_INVALID_ARG, "table was built on device %d", h->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t pt = h->is_g2 ? GPBC_G2_BYTES : GPBC_G1_BYTES;
    std::vector<OpnBlock> blocks(n_blocks);
    opn_blocks(seg_off, k, blocks.data());
    Scratch tmp;
    TRY(tmp.open(st, 0, Scratch::padded(n_blocks * sizeof(OpnBlock))));
    OpnBlock *d_blocks = tmp.take<OpnBlock>(n_blocks * sizeof(OpnBlock));
    TRY(upload_table_async(blocks.data(), n_blocks * sizeof(OpnBlock), d_blocks, st));
    uint8_t *partial = n_chunks > 1 ? (uint8_t *)d_workspace : (uint8_t *)d_out;
    // with chunks to add, the deciding lanes leave their flags where the mask finds them: the caller's ok_out, or the workspace's tail
    uint8_t *flags = n_chunks > 1 && !d_ok_out ? (uint8_t *)d_workspace + openings_partial_bytes(h, n) : d_ok_out;
    const unsigned grid = (unsigned)(n_blocks * n_chunks);
    const uint8_t *cf = (const uint8_t *)d_coeffs, *id = (const uint8_t *)d_ids;
    const bool small = m_max <= (size_t)OPN_SMALL_M;
    if (h->is_g2 && small) TRY(GPBC_LAUNCH(k_g2_fb_openings, grid, BLOCK, st, h->table, h->base_inf, h->nbase, cf, id, d_blocks, (uint32_t)n_blocks, n, (uint32_t)C, partial, flags));
    else if (h->is_g2) TRY(GPBC_LAUNCH(k_g2_fb_openings_long, grid, BLOCK, st, h->table, h->base_inf, h->nbase, cf, id, d_blocks, (uint32_t)n_blocks, n, (uint32_t)C, partial, flags));
    else if (small) TRY(GPBC_LAUNCH(k_g1_fb_openings, grid, BLOCK, st, h->table, h->base_inf, h->nbase, cf, id, d_blocks, (uint32_t)n_blocks, n, (uint32_t)C, partial, flags));
    else TRY(GPBC_LAUNCH(k_g1_fb_openings_long, grid, BLOCK, st, h->table, h->base_inf, h->nbase, cf, id, d_blocks, (uint32_t)n_blocks, n, (uint32_t)C, partial, flags));
    if (n_chunks == 1) return GPBC_OK;
    // partials are chunk-major (partial[c * n + i]); as in gpbc_fixed_base_msm_dev every launch of the strided sum divides the number of
    // chunks by 16 until one row per identity is left
    const uint8_t *in = partial;
    uint8_t *ws = partial + n_chunks * n * pt;
    for (size_t c = n_chunks; c > 1;) {
        const size_t c2 = (c + 15) / 16;
        uint8_t *o = c2 == 1 ? (uint8_t *)d_out : ws;
        TRY(point_sum_strided_dev(h->is_g2 != 0, in, c * n, o, c2 * n, st));
        in = o; ws += c2 * n * pt; c = c2;
    }
    return GPBC_LAUNCH(k_fb_openings_mask, grid_for(n * (pt / 4)), BLOCK, st, flags, n, (uint32_t)(pt / 4), (uint32_t *)d_out);
}
// Host pointers: the shared staging path on the table's device only (the handle lives there), neither combined nor cut: a segment's
// identities share their polynomial's row.
int gpbc_fixed_base_openings(const gpbc_fixed_base *h, const void *coeffs, const void *ids, const uint64_t *seg_off, size_t k, void *out, uint8_t *ok_out) {
    if (!k) return h ? GPBC_OK : fail(GPBC_ERR_INVALID_ARG, "null table handle");
    size_t n = 0, m_max = 0;
    TRY(openings_args(h, coeffs, ids, seg_off, k, out, ok_out, &n, &m_max));
    if (!n) return GPBC_OK;
    TRY(bind_device());
    if (current_device() != h->device) return fail(GPBC_ERR_INVALID_ARG, "table was built on device %d", h->device);
    HostCall c = HostCall().input(coeffs, k * h->nbase * GPBC_SCALAR_BYTES, true).input(ids, GPBC_SCALAR_BYTES).output(out, h->is_g2 ? GPBC_G2_BYTES : GPBC_G1_BYTES);
    if (ok_out) c.output(ok_out, 1);
    const bool has_ok = ok_out != nullptr;
    const size_t wsb = gpbc_fixed_base_openings_workspace_bytes(h, n);
    return host_call(n, c, HostRoute{CALL_KINDS, nullptr, 0, 0, 0, wsb},
                     [=](const DevCols &d, size_t, hipStream_t st) { return gpbc_fixed_base_openings_dev(h, d.in[0], d.in[1], seg_off, k, d.out[0], has_ok ? d.out[1] : nullptr, d.tmp, wsb, st); });
}

}  // extern "C"
