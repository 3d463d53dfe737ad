// libgpbc_bn254.so, one of the units listed in _build.py: the row form of gpbc_g1 / g2_scalar_mul_batch(_dev) — 1 < nbase < n, one base
// per row of m = n / nbase scalars (csrc/rows29.hip.hpp).  No C-ABI entry of its own: gpbc_curve.hip's entries reach it through
// scalar_mul_rows_dev (gpbc_common.hpp).  gfx950 only.
// A unit of its own, and not beside k_g1_scalar_mul in gpbc_curve.hip: every older unit stays the parent's device code (DESIGN.md,
// "Per-row shared-base scalar multiplication"); the price is another copy of the scalar-multiplication loops in the library.
#include <cstdlib>
#include "gpbc_common.hpp"
#include "rows29.hip.hpp"

// The table-free rows: lane t of a chunk owns output first + t and loads base (first + t) / m
GPBC_KERNEL_G1 k_g1_rows_free(const uint8_t *__restrict__ bases, size_t m, const uint8_t *__restrict__ scalars, uint8_t *__restrict__ out, size_t first, size_t count,
                              int32_t *__restrict__ tabws) {
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= count) return;
    const size_t i = first + t;
    uint32_t k[8];
    load_scalar(k, scalars + i * GPBC_SCALAR_BYTES);
    AffP<Fe> r;
    rows_free_lane<Fe>(r, g1_load_aff(bases + (i / m) * GPBC_G1_BYTES), k, tabws + t * (size_t)glv_table_dwords<Fe>());
    g1_store_aff(out + i * GPBC_G1_BYTES, r);
}
GPBC_KERNEL k_g2_rows_free(const uint8_t *__restrict__ bases, size_t m, const uint8_t *__restrict__ scalars, uint8_t *__restrict__ out, size_t first, size_t count,
                           int32_t *__restrict__ tabws) {
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= count) return;
    const size_t i = first + t;
    uint32_t k[8];
    load_scalar(k, scalars + i * GPBC_SCALAR_BYTES);
    AffP<F2> r;
    rows_free_lane<F2>(r, g2_load_aff(bases + (i / m) * GPBC_G2_BYTES), k, tabws + t * (size_t)glv_table_dwords<F2>());
    g2_store_aff(out + i * GPBC_G2_BYTES, r);
}

// The G1 row tables.  Build (a) for a group of nb bases: wb = nb x 32 rows of window bases, inf = nb flags; build (b) for a pass of nb
// of them: table = nb x 480 rows.
GPBC_KERNEL_G1 k_g1_rows_build_a(const uint8_t *__restrict__ bases, size_t nb, int32_t *__restrict__ wb, uint8_t *__restrict__ inf) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= nb) return;
    rows_build_a_lane(g1_load_aff(bases + j * GPBC_G1_BYTES), wb + j * (size_t)ROWS_WINDOWS * ROWS_ENTRY_DWORDS, inf + j);
}
GPBC_KERNEL_G1 k_g1_rows_build_b(const int32_t *__restrict__ wb, int32_t *__restrict__ table, const uint8_t *__restrict__ inf, size_t nb) {
    const size_t q = (size_t)blockIdx.x * BLOCK + threadIdx.x, j = q / ROWS_WINDOWS;
    if (j >= nb) return;
    rows_build_b_lane(wb + j * (size_t)ROWS_WINDOWS * ROWS_ENTRY_DWORDS, table + j * (size_t)ROWS_ENTRIES * ROWS_ENTRY_DWORDS, inf + j, (int)(q % ROWS_WINDOWS));
}
// one lane per output of the pass; a wave may straddle two bases, each lane addresses its own base's rows
GPBC_KERNEL_G1 k_g1_rows_eval(const int32_t *__restrict__ table, const uint8_t *__restrict__ inf, size_t m, const uint8_t *__restrict__ scalars, uint8_t *__restrict__ out, size_t count) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= count) return;
    const size_t j = i / m;
    uint32_t k[8];
    load_scalar(k, scalars + i * GPBC_SCALAR_BYTES);
    JacP<Fe> acc;
    rows_eval_lane(acc, table + j * (size_t)ROWS_ENTRIES * ROWS_ENTRY_DWORDS, inf[j] != 0, k);
    AffP<Fe> r;
    jac_to_affine(r, acc);
    g1_store_aff(out + i * GPBC_G1_BYTES, r);
}

static int rows_free_dev(bool g2, const uint8_t *d_bases, size_t m, const uint8_t *d_scalars, size_t n, uint8_t *d_out, hipStream_t st) {
    const size_t tab_bytes = sizeof(int32_t) * (g2 ? (size_t)glv_table_dwords<F2>() : (size_t)glv_table_dwords<Fe>());
    const size_t chunk = n < SMUL_CHUNK ? n : SMUL_CHUNK;
    std::lock_guard<std::mutex> seq(g_ws_seq_mu);
    int32_t *tabws = nullptr;
    TRY(stream_workspace(st, chunk * tab_bytes, &tabws));
    for (size_t off = 0; off < n; off += chunk) {
        const size_t c = n - off < chunk ? n - off : chunk;
        if (g2) TRY(GPBC_LAUNCH(k_g2_rows_free, grid_for(c), BLOCK, st, d_bases, m, d_scalars, d_out, off, c, tabws));
        else TRY(GPBC_LAUNCH(k_g1_rows_free, grid_for(c), BLOCK, st, d_bases, m, d_scalars, d_out, off, c, tabws));
    }
    return GPBC_OK;
}

// GPBC_ERR_WORKSPACE: the tables' memory could not be had, nothing was enqueued
static int rows_table_dev(const uint8_t *d_bases, size_t nbase, size_t m, const uint8_t *d_scalars, uint8_t *d_out, hipStream_t st) {
    const size_t pass = rows_pass_bases(nbase, m), group = nbase < ROWS_GROUP_BASES ? nbase : ROWS_GROUP_BASES;
    Scratch tmp;
    if (tmp.open(st, 0, Scratch::padded(pass * ROWS_TABLE_BYTES) + Scratch::padded(group * ROWS_WB_BYTES) + Scratch::padded(group)) != GPBC_OK) return GPBC_ERR_WORKSPACE;
    int32_t *table = tmp.take<int32_t>(pass * ROWS_TABLE_BYTES), *wb = tmp.take<int32_t>(group * ROWS_WB_BYTES);
    uint8_t *inf = tmp.take(group);
    for (size_t g0 = 0; g0 < nbase; g0 += group) {
        const size_t ng = nbase - g0 < group ? nbase - g0 : group;
        TRY(GPBC_LAUNCH(k_g1_rows_build_a, grid_for(ng), BLOCK, st, d_bases + g0 * GPBC_G1_BYTES, ng, wb, inf));
        for (size_t p0 = 0; p0 < ng; p0 += pass) {
            const size_t nb = ng - p0 < pass ? ng - p0 : pass, b0 = g0 + p0;
            TRY(GPBC_LAUNCH(k_g1_rows_build_b, grid_for(nb * ROWS_WINDOWS), BLOCK, st, wb + p0 * (size_t)ROWS_WINDOWS * ROWS_ENTRY_DWORDS, table, inf + p0, nb));
            TRY(GPBC_LAUNCH(k_g1_rows_eval, grid_for(nb * m), BLOCK, st, table, inf + p0, m, d_scalars + b0 * m * GPBC_SCALAR_BYTES, d_out + b0 * m * GPBC_G1_BYTES, nb * m));
        }
    }
    return GPBC_OK;
}

// GPBC_ROWS_TABLE_MIN in the environment replaces ROWS_TABLE_MIN for the call (tools/scalar_mul_rows_bench.py: 2 takes the tables at
// every row length they serve, 0 never takes them); the results do not depend on it.
static size_t rows_table_min() {
    const char *e = getenv("GPBC_ROWS_TABLE_MIN");
    if (!e || !*e) return ROWS_TABLE_MIN;
    const unsigned long long v = strtoull(e, nullptr, 10);
    return v ? (size_t)v : ~(size_t)0;
}

// out[j m + i] = [scalars[j m + i]] bases[j], j < nbase, i < m; the caller has checked the arguments and bound the device.  G1 rows of
// ROWS_TABLE_MIN .. table_max - 1 scalars and G2 rows of ROWS_G2_TABLE_MIN .. table_max - 1 (gpbc_rows_g2.hip) take their group's row
// tables (and the table-free kernel when their memory cannot be had), every other row the table-free kernel.  Asynchronous on `st`.
int scalar_mul_rows_dev(bool g2, const void *d_bases, size_t nbase, const void *d_scalars, size_t m, void *d_out, size_t table_max, hipStream_t st) {
    if (!nbase || !m) return GPBC_OK;
    if (m >= (g2 ? rows_g2_table_min() : rows_table_min()) && m < table_max) {
        const int rc = g2 ? rows_g2_table_dev(d_bases, nbase, m, d_scalars, d_out, st)
                          : rows_table_dev((const uint8_t *)d_bases, nbase, m, (const uint8_t *)d_scalars, (uint8_t *)d_out, st);
        if (rc != GPBC_ERR_WORKSPACE) return rc;
    }
    return rows_free_dev(g2, (const uint8_t *)d_bases, m, (const uint8_t *)d_scalars, nbase * m, (uint8_t *)d_out, st);
}
