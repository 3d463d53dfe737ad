// libgpbc_bn254.so, one of the units listed in _build.py: bit-selected sums over a fixed set in G1 / G2 — the subset-sum tables over the bit string and the
// sums over them (csrc/subset29.hip.hpp) with their C-ABI entries (include/gpbc_bn254_subset.h).  gfx950 only.
#include "gpbc_common.hpp"
#include "../../include/gpbc_bn254_subset.h"
#include "subset29.hip.hpp"

template <class F> struct SubsetPoint;
template <> struct SubsetPoint<Fe> {
    static constexpr size_t BYTES = GPBC_G1_BYTES;
    static __device__ __forceinline__ AffP<Fe> load(const uint8_t *p) { return g1_load_aff(p); }
    static __device__ __forceinline__ void store(uint8_t *p, const AffP<Fe> &r) { g1_store_aff(p, r); }
};
template <> struct SubsetPoint<F2> {
    static constexpr size_t BYTES = GPBC_G2_BYTES;
    static __device__ __forceinline__ AffP<F2> load(const uint8_t *p) { return g2_load_aff(p); }
    static __device__ __forceinline__ void store(uint8_t *p, const AffP<F2> &r) { g2_store_aff(p, r); }
};

// one lane per table entry e = w * 256 + v
template <class F> __device__ __forceinline__ void subset_build_lane(const uint8_t *bases, size_t nbits, const uint8_t *offset, int32_t *table, uint8_t *flags) {
    const size_t e = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= subset_entries(nbits)) return;
    using Pt = SubsetPoint<F>;
    AffP<F> off, a;
    if (offset && e < 256) off = Pt::load(offset);
    subset_entry<F>(a, [&](size_t i) { return Pt::load(bases + i * Pt::BYTES); }, nbits, offset ? &off : nullptr, e >> 8, (int)(e & 255));
    subset_entry_store<F>(table, flags, e, a);
}
GPBC_KERNEL_G1 k_g1_subset_build(const uint8_t *__restrict__ bases, size_t nbits, const uint8_t *__restrict__ offset, int32_t *__restrict__ table, uint8_t *__restrict__ flags) {
    subset_build_lane<Fe>(bases, nbits, offset, table, flags);
}
GPBC_KERNEL k_g2_subset_build(const uint8_t *__restrict__ bases, size_t nbits, const uint8_t *__restrict__ offset, int32_t *__restrict__ table, uint8_t *__restrict__ flags) {
    subset_build_lane<F2>(bases, nbits, offset, table, flags);
}

// lane t = c * n + m: windows [c * C, (c + 1) * C) of item m -> partial[t] (chunk-major; with one chunk partial is the output)
template <class F> __device__ __forceinline__ void subset_sum_lane(const int32_t *table, const uint8_t *flags, const uint8_t *masks, size_t n, size_t W, size_t C,
                                                                   size_t n_chunks, uint8_t *partial) {
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n * n_chunks) return;
    const size_t m = t % n, c = t / n;
    JacP<F> acc = subset_lane<F>(table, flags, masks + m * W, W, c * C, C);
    AffP<F> a;
    jac_to_affine(a, acc);
    SubsetPoint<F>::store(partial + t * SubsetPoint<F>::BYTES, a);
}
GPBC_KERNEL_G1 k_g1_subset_sum(const int32_t *__restrict__ table, const uint8_t *__restrict__ flags, const uint8_t *__restrict__ masks, size_t n, size_t W, size_t C,
                               size_t n_chunks, uint8_t *__restrict__ partial) {
    subset_sum_lane<Fe>(table, flags, masks, n, W, C, n_chunks, partial);
}
GPBC_KERNEL k_g2_subset_sum(const int32_t *__restrict__ table, const uint8_t *__restrict__ flags, const uint8_t *__restrict__ masks, size_t n, size_t W, size_t C,
                            size_t n_chunks, uint8_t *__restrict__ partial) {
    subset_sum_lane<F2>(table, flags, masks, n, W, C, n_chunks, partial);
}

struct gpbc_subset_table { int device; int is_g2; size_t nbits, W; int32_t *table; uint8_t *flags; };

static size_t subset_row_bytes(int is_g2) { return sizeof(int32_t) * (is_g2 ? (size_t)TabLayout<F2>::ENTRY_DWORDS : (size_t)TabLayout<Fe>::ENTRY_DWORDS); }
static size_t subset_point_bytes(int is_g2) { return is_g2 ? GPBC_G2_BYTES : GPBC_G1_BYTES; }
static int subset_check_create(const void *bases, size_t nbits, gpbc_subset_table **out) {
    if (!out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    *out = nullptr;
    if (!nbits || !bases) return fail(GPBC_ERR_INVALID_ARG, "a subset table needs at least one base");
    if (nbits > SUBSET_MAX_BITS) return fail(GPBC_ERR_INVALID_ARG, "nbits = %zu is above the cap of %zu (a table of %zu windows)", nbits, SUBSET_MAX_BITS, subset_windows(SUBSET_MAX_BITS));
    return GPBC_OK;
}

extern "C" {

int gpbc_subset_version(void) { return 1; }
size_t gpbc_subset_table_bytes(size_t nbits, int is_g2) {
    if (!nbits || nbits > SUBSET_MAX_BITS) return 0;
    return subset_entries(nbits) * (subset_row_bytes(is_g2) + 1);
}
int gpbc_subset_table_create_dev(int is_g2, const void *d_bases, size_t nbits, const void *d_offset, void *stream, gpbc_subset_table **out) {
    TRY(subset_check_create(d_bases, nbits, out));
    TRY(bind_device());
    const size_t entries = subset_entries(nbits);
    gpbc_subset_table *h = new gpbc_subset_table{current_device(), is_g2 ? 1 : 0, nbits, subset_windows(nbits), nullptr, nullptr};
    hipError_t e1 = hipMalloc((void **)&h->table, entries * subset_row_bytes(is_g2));
    hipError_t e2 = e1 == hipSuccess ? hipMalloc((void **)&h->flags, entries) : e1;
    if (e1 != hipSuccess || e2 != hipSuccess) {
        if (h->table) (void)hipFree(h->table);
        delete h;
        return fail(GPBC_ERR_HIP, "hipMalloc of a %zu-byte subset table failed", gpbc_subset_table_bytes(nbits, is_g2));
    }
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (is_g2) rc = GPBC_LAUNCH(k_g2_subset_build, grid_for(entries), BLOCK, st, (const uint8_t *)d_bases, nbits, (const uint8_t *)d_offset, h->table, h->flags);
    else rc = GPBC_LAUNCH(k_g1_subset_build, grid_for(entries), BLOCK, st, (const uint8_t *)d_bases, nbits, (const uint8_t *)d_offset, h->table, h->flags);
    if (rc != GPBC_OK) { (void)hipFree(h->table); (void)hipFree(h->flags); delete h; return rc; }
    *out = h;
    return GPBC_OK;
}
static int subset_create_host(int is_g2, const void *bases, size_t nbits, const void *offset, gpbc_subset_table **out) {
    TRY(subset_check_create(bases, nbits, out));
    TRY(bind_device());
    DevBuf dB, dO;
    TRY(dB.upload(bases, nbits * subset_point_bytes(is_g2)));
    if (offset) TRY(dO.upload(offset, subset_point_bytes(is_g2)));
    TRY(gpbc_subset_table_create_dev(is_g2, dB.p, nbits, offset ? dO.p : nullptr, nullptr, out));
    const int rc = sync_default();                                   // the point buffers are freed on return
    if (rc != GPBC_OK) { (void)gpbc_subset_table_destroy(*out); *out = nullptr; }
    return rc;
}
int gpbc_g1_subset_table_create(const void *bases, size_t nbits, const void *offset, gpbc_subset_table **out) { return subset_create_host(0, bases, nbits, offset, out); }
int gpbc_g2_subset_table_create(const void *bases, size_t nbits, const void *offset, gpbc_subset_table **out) { return subset_create_host(1, bases, nbits, offset, out); }
int gpbc_subset_table_destroy(gpbc_subset_table *t) {
    if (!t) return GPBC_OK;
    (void)hipSetDevice(t->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(t->table);
    (void)hipFree(t->flags);
    delete t;
    return GPBC_OK;
}
// the chunk-major partial sums; nothing for one chunk (the lanes write the output)
size_t gpbc_subset_sum_workspace_bytes(const gpbc_subset_table *t, size_t n) {
    if (!t || !n) return 0;
    size_t C, n_chunks;
    subset_shape(t->W, n, C, n_chunks);
    return n_chunks > 1 ? n_chunks * n * subset_point_bytes(t->is_g2) : 0;
}
int gpbc_subset_sum_dev(const gpbc_subset_table *t, const void *d_masks, size_t n, void *d_out, void *d_workspace, size_t workspace_bytes, void *stream) {
    if (!t) return fail(GPBC_ERR_INVALID_ARG, "null table handle");
    if (!n) return GPBC_OK;
    if (!d_masks || !d_out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    size_t C, n_chunks;
    subset_shape(t->W, n, C, n_chunks);
    const size_t need = gpbc_subset_sum_workspace_bytes(t, n);
    if (need && (!d_workspace || workspace_bytes < need))
        return fail(GPBC_ERR_INVALID_ARG, "workspace too small: %zu bytes given, %zu needed (gpbc_subset_sum_workspace_bytes)", d_workspace ? workspace_bytes : (size_t)0, need);
    TRY(bind_device());
    if (current_device() != t->device) return fail(GPBC_ERR_INVALID_ARG, "table was built on device %d", t->device);
    hipStream_t st = (hipStream_t)stream;
    uint8_t *partial = n_chunks > 1 ? (uint8_t *)d_workspace : (uint8_t *)d_out;
    const size_t lanes = n * n_chunks;
    if (t->is_g2) TRY(GPBC_LAUNCH(k_g2_subset_sum, grid_for(lanes), BLOCK, st, t->table, t->flags, (const uint8_t *)d_masks, n, t->W, C, n_chunks, partial));
    else TRY(GPBC_LAUNCH(k_g1_subset_sum, grid_for(lanes), BLOCK, st, t->table, t->flags, (const uint8_t *)d_masks, n, t->W, C, n_chunks, partial));
    if (n_chunks > 1) TRY(point_sum_strided_dev(t->is_g2 != 0, partial, lanes, d_out, n, st));       // out[m] = sum_c partial[c * n + m]
    return GPBC_OK;
}
// Host pointers: the shared staging path (host_call) — a call of up to LANE_CALL_MAX_UNITS items on a call lane of its own, a larger one
// through device blocks; not combined with other threads' calls, and on the table's device only.
int gpbc_subset_sum(const gpbc_subset_table *t, const void *masks, size_t n, void *out) {
    if (!t) return fail(GPBC_ERR_INVALID_ARG, "null table handle");
    if (!n) return GPBC_OK;
    if (!masks || !out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    const size_t wsb = gpbc_subset_sum_workspace_bytes(t, n);
    return host_call(n, HostCall().input(masks, t->W).output(out, subset_point_bytes(t->is_g2)), HostRoute{CALL_KINDS, nullptr, 0, LANE_CALL_MAX_UNITS, 0, wsb},
                     [=](const DevCols &d, size_t m, hipStream_t st) { return gpbc_subset_sum_dev(t, d.in[0], m, d.out[0], d.tmp, wsb, st); });
}

}  // extern "C"
