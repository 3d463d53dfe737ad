// libgpbc_bn254.so, the thirteenth unit (_build.GTFIXED_SOURCES): window tables of public GT elements and indexed products of their powers
// (csrc/gtfixed29.hip.hpp) with the C-ABI entries of include/gpbc_bn254_gtfixed.h.  gfx950 only.
// A unit of its own, and not beside k_gt_exp in gpbc_pairing.hip or the multi-exponentiation in gpbc_gtmexp.hip: kernels added to the
// pairing unit changed the compiler's schedule of k_final_exp (profiles/membership_bench_ab.txt).  Here every older unit is the parent's
// source and compiles to the parent's code; the price is another copy of f12p_mul and f12p_sqr in the library.
#include "gpbc_common.hpp"
#include "gtfixed29.hip.hpp"
#include "../../include/gpbc_bn254_gtfixed.h"

static_assert(GPBC_INDEX_NONE == FBI_NONE && GPBC_GT_BYTES == 384, "gtfixed29.hip.hpp restates the index convention and the element size");

// One lane pair per (base, window): pair q builds window q % 32 of base q / 32, so a wavefront is the 32 windows of one base and its
// pairs run the squarings in step (w_max = 31).  The pairs past the last base return together.
GPBC_KERNEL k_gt_fb_build(const uint8_t *__restrict__ bases, size_t nbase, int32_t *__restrict__ table) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x, q = lane >> 1;
    const size_t j = q / GTFB_WINDOWS;
    if (j >= nbase) return;
    const int w = (int)(q % GTFB_WINDOWS);
    PairDpp x{(bool)(lane & 1)};
    gt_fb_build_lane(x, bases + j * GPBC_GT_BYTES + (x.odd ? 192 : 0), w, GTFB_WINDOWS - 1, table + j * GTFB_BASE_DWORDS + (size_t)w * GTFB_WINDOW_DWORDS);
}

// One output per lane pair, the lane layout of k_gt_exp (even lane C0, odd lane C1).  The pair past the last output returns together.
GPBC_KERNEL k_gt_fb_indexed(const int32_t *__restrict__ table, size_t nbase, const uint32_t *__restrict__ index, size_t n_index_rows, uint32_t terms,
                            const uint8_t *__restrict__ scalars, size_t n, uint8_t *__restrict__ out, uint8_t *__restrict__ ok) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x, i = lane >> 1;
    if (i >= n) return;
    PairDpp x{(bool)(lane & 1)};
    gt_fb_indexed_lane(x, table, nbase, index + (i % n_index_rows) * terms, terms, scalars + i * (size_t)terms * GPBC_SCALAR_BYTES,
                       out + i * GPBC_GT_BYTES + (x.odd ? 192 : 0), ok ? ok + i : nullptr, [](uint32_t *k, const uint8_t *p) { load_scalar(k, p); });
}

struct gpbc_gt_fixed_base { int device; size_t nbase; int32_t *table; };

extern "C" {

int gpbc_gtfixed_version(void) { return 1; }

size_t gpbc_gt_fixed_base_table_bytes(size_t nbase) {
    const size_t per_base = GTFB_BASE_DWORDS * sizeof(int32_t);
    return nbase > ~(size_t)0 / per_base ? 0 : nbase * per_base;
}
int gpbc_gt_fixed_base_create_dev(const void *d_bases, size_t nbase, void *stream, gpbc_gt_fixed_base **out) {
    if (!out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    *out = nullptr;
    if (!nbase || !d_bases) return fail(GPBC_ERR_INVALID_ARG, "fixed-base table needs at least one base");
    // an index is a uint32 and GPBC_INDEX_NONE is not a base; 2 * 32 * nbase lanes must fit the grid
    if (nbase >= (size_t)1 << 24 || !gpbc_gt_fixed_base_table_bytes(nbase)) return fail(GPBC_ERR_INVALID_ARG, "too many bases for one table (%zu)", nbase);
    TRY(bind_device());
    gpbc_gt_fixed_base *h = new gpbc_gt_fixed_base{current_device(), nbase, nullptr};
    if (hipMalloc((void **)&h->table, gpbc_gt_fixed_base_table_bytes(nbase)) != hipSuccess) {
        delete h;
        return fail(GPBC_ERR_HIP, "hipMalloc of a %zu-byte fixed-base table failed", gpbc_gt_fixed_base_table_bytes(nbase));
    }
    const int rc = GPBC_LAUNCH(k_gt_fb_build, grid_for(2 * GTFB_WINDOWS * nbase), BLOCK, (hipStream_t)stream, (const uint8_t *)d_bases, nbase, h->table);
    if (rc != GPBC_OK) { (void)hipFree(h->table); delete h; return rc; }
    *out = h;
    return GPBC_OK;
}
int gpbc_gt_fixed_base_create(const void *bases, size_t nbase, gpbc_gt_fixed_base **out) {
    if (!out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    *out = nullptr;
    if (!nbase || !bases) return fail(GPBC_ERR_INVALID_ARG, "fixed-base table needs at least one base");
    if (nbase >= (size_t)1 << 24) return fail(GPBC_ERR_INVALID_ARG, "too many bases for one table (%zu)", nbase);
    TRY(bind_device());
    DevBuf dB;
    TRY(dB.upload(bases, nbase * GPBC_GT_BYTES));
    TRY(gpbc_gt_fixed_base_create_dev(dB.p, nbase, nullptr, out));
    const int rc = sync_default();                                   // the bases buffer is freed on return
    if (rc != GPBC_OK) { (void)gpbc_gt_fixed_base_destroy(*out); *out = nullptr; }
    return rc;
}
int gpbc_gt_fixed_base_destroy(gpbc_gt_fixed_base *h) {
    if (!h) return GPBC_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(h->table);
    delete h;
    return GPBC_OK;
}

// Everything that can be said without the device: the limits, then the pointers and their ranges (an output row is 384 bytes whatever
// the table), then the handle — a null handle is refused also where there is nothing to do, as gpbc_fixed_base_indexed refuses it.
static int gtfb_indexed_args(const gpbc_gt_fixed_base *h, const uint32_t *index, size_t n_index_rows, size_t terms, const void *scalars, size_t n, const void *out, const uint8_t *ok_out) {
    if (terms < 1 || terms > FBI_MAX_TERMS) return fail(GPBC_ERR_INVALID_ARG, "terms must be in 1 .. %zu (got %zu)", FBI_MAX_TERMS, terms);
    if (n > (size_t)0xffffffffu / terms) return fail(GPBC_ERR_INVALID_ARG, "n * terms must stay below 2^32 (got n = %zu, terms = %zu)", n, terms);
    if (n) {
        if (n_index_rows < 1 || n_index_rows > n) return fail(GPBC_ERR_INVALID_ARG, "n_index_rows must be in 1 .. n (got %zu, n = %zu)", n_index_rows, n);
        if (!index || !scalars || !out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
        const ByteRange r[4] = {{index, n_index_rows * terms * sizeof(uint32_t)}, {scalars, n * terms * GPBC_SCALAR_BYTES}, {out, n * GPBC_GT_BYTES}, {ok_out, n}};
        if (outputs_overlap(r, 2, 4))
            return fail(GPBC_ERR_INVALID_ARG, "an output overlaps an input or the other output");
    }
    if (!h) return fail(GPBC_ERR_INVALID_ARG, "null table handle");
    return GPBC_OK;
}
int gpbc_gt_fixed_base_indexed_dev(const gpbc_gt_fixed_base *h, const uint32_t *d_index, size_t n_index_rows, size_t terms, const void *d_scalars, size_t n, void *d_out,
                                   uint8_t *d_ok_out, void *stream) {
    TRY(gtfb_indexed_args(h, d_index, n_index_rows, terms, d_scalars, n, d_out, d_ok_out));
    if (!n) return GPBC_OK;
    TRY(bind_device());
    if (current_device() != h->device) return fail(GPBC_ERR_INVALID_ARG, "table was built on device %d", h->device);
    return GPBC_LAUNCH(k_gt_fb_indexed, grid_for(2 * n), BLOCK, (hipStream_t)stream, h->table, h->nbase, d_index, n_index_rows, (uint32_t)terms, (const uint8_t *)d_scalars, n,
                       (uint8_t *)d_out, d_ok_out);
}
// Host pointers: the shared staging path on the table's device only (the handle lives there), not combined with other threads' calls and
// not cut into chunks (a periodic index row belongs to an output by its position in the whole call).
int gpbc_gt_fixed_base_indexed(const gpbc_gt_fixed_base *h, const uint32_t *index, size_t n_index_rows, size_t terms, const void *scalars, size_t n, void *out, uint8_t *ok_out) {
    TRY(gtfb_indexed_args(h, index, n_index_rows, terms, scalars, n, out, ok_out));
    if (!n) return GPBC_OK;
    TRY(bind_device());
    if (current_device() != h->device) return fail(GPBC_ERR_INVALID_ARG, "table was built on device %d", h->device);
    const bool own = n_index_rows == n;
    HostCall c = HostCall().input(scalars, terms * GPBC_SCALAR_BYTES);
    if (own) c.input(index, terms * sizeof(uint32_t)); else c.input(index, n_index_rows * terms * sizeof(uint32_t), true);
    c.output(out, GPBC_GT_BYTES);
    if (ok_out) c.output(ok_out, 1);
    const bool has_ok = ok_out != nullptr;
    return host_call(n, c, HostRoute{CALL_KINDS, nullptr, 0, LANE_CALL_MAX_UNITS},
                     [=](const DevCols &d, size_t m, hipStream_t st) {
                         return gpbc_gt_fixed_base_indexed_dev(h, (const uint32_t *)d.in[1], own ? m : n_index_rows, terms, d.in[0], m, d.out[0], has_ok ? d.out[1] : nullptr, st);
                     });
}

}  // extern "C"
