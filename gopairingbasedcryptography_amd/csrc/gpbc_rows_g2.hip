// libgpbc_bn254.so, one of the units listed in _build.py: the G2 row tables of the row form of gpbc_g2_scalar_mul_batch(_dev) — 1 < nbase < n,
// one base per row of m = n / nbase scalars (csrc/rows29_g2.hip.hpp).  No C-ABI entry of its own: scalar_mul_rows_dev (gpbc_rows.hip)
// reaches it through rows_g2_table_dev (gpbc_common.hpp).  gfx950 only.
// A unit of its own, and not beside the G1 tables in gpbc_rows.hip: every older unit stays the parent's device code ("G2 row
// tables over the GLS split").
#include <cstdlib>
#include "gpbc_common.hpp"
#include "rows29_g2.hip.hpp"

constexpr size_t G2_WB_DWORDS = (size_t)ROWS_G2_WINDOWS * ROWS_G2_ENTRY_DWORDS, G2_BASE_DWORDS = (size_t)ROWS_G2_ENTRIES * ROWS_G2_ENTRY_DWORDS;

// Build (a) for a group of nb bases: wb = nb x 17 rows of window bases, inf = nb flags; build (b) for a pass of nb of them: table =
// nb x 255 rows.
GPBC_KERNEL k_g2_rows_build_a(const uint8_t *__restrict__ bases, size_t nb, int32_t *__restrict__ wb, uint8_t *__restrict__ inf) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= nb) return;
    rows_g2_build_a_lane(g2_load_aff(bases + j * GPBC_G2_BYTES), wb + j * G2_WB_DWORDS, inf + j);
}
GPBC_KERNEL k_g2_rows_build_b(const int32_t *__restrict__ wb, int32_t *__restrict__ table, const uint8_t *__restrict__ inf, size_t nb) {
    const size_t q = (size_t)blockIdx.x * BLOCK + threadIdx.x, j = q / ROWS_G2_WINDOWS;
    if (j >= nb) return;
    rows_g2_build_b_lane(wb + j * G2_WB_DWORDS, table + j * G2_BASE_DWORDS, inf + j, (int)(q % ROWS_G2_WINDOWS));
}
// one lane per output of the pass; a wave may straddle two bases, each lane addresses its own base's rows
GPBC_KERNEL k_g2_rows_eval(const int32_t *__restrict__ table, const uint8_t *__restrict__ inf, size_t m, const uint8_t *__restrict__ scalars, uint8_t *__restrict__ out, size_t count) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= count) return;
    const size_t j = i / m;
    uint32_t k[8];
    load_scalar(k, scalars + i * GPBC_SCALAR_BYTES);
    JacP<F2> acc;
    rows_g2_eval_lane(acc, table + j * G2_BASE_DWORDS, inf[j] != 0, k);
    AffP<F2> r;
    jac_to_affine(r, acc);
    g2_store_aff(out + i * GPBC_G2_BYTES, r);
}

// GPBC_ERR_WORKSPACE: the tables' memory could not be had, nothing was enqueued
int rows_g2_table_dev(const void *d_bases_, size_t nbase, size_t m, const void *d_scalars_, void *d_out_, hipStream_t st) {
    const uint8_t *d_bases = (const uint8_t *)d_bases_, *d_scalars = (const uint8_t *)d_scalars_;
    uint8_t *d_out = (uint8_t *)d_out_;
    const size_t pass = rows_g2_pass_bases(nbase, m), group = nbase < ROWS_G2_GROUP_BASES ? nbase : ROWS_G2_GROUP_BASES;
    Scratch tmp;
    if (tmp.open(st, 0, Scratch::padded(pass * ROWS_G2_TABLE_BYTES) + Scratch::padded(group * ROWS_G2_WB_BYTES) + Scratch::padded(group)) != GPBC_OK) return GPBC_ERR_WORKSPACE;
    int32_t *table = tmp.take<int32_t>(pass * ROWS_G2_TABLE_BYTES), *wb = tmp.take<int32_t>(group * ROWS_G2_WB_BYTES);
    uint8_t *inf = tmp.take(group);
    for (size_t g0 = 0; g0 < nbase; g0 += group) {
        const size_t ng = nbase - g0 < group ? nbase - g0 : group;
        TRY(GPBC_LAUNCH(k_g2_rows_build_a, grid_for(ng), BLOCK, st, d_bases + g0 * GPBC_G2_BYTES, ng, wb, inf));
        for (size_t p0 = 0; p0 < ng; p0 += pass) {
            const size_t nb = ng - p0 < pass ? ng - p0 : pass, b0 = g0 + p0;
            TRY(GPBC_LAUNCH(k_g2_rows_build_b, grid_for(nb * ROWS_G2_WINDOWS), BLOCK, st, wb + p0 * G2_WB_DWORDS, table, inf + p0, nb));
            TRY(GPBC_LAUNCH(k_g2_rows_eval, grid_for(nb * m), BLOCK, st, table, inf + p0, m, d_scalars + b0 * m * GPBC_SCALAR_BYTES, d_out + b0 * m * GPBC_G2_BYTES, nb * m));
        }
    }
    return GPBC_OK;
}

// GPBC_ROWS_G2_TABLE_MIN in the environment replaces ROWS_G2_TABLE_MIN for the call (tools/scalar_mul_rows_g2_bench.py: 2 takes the tables
// at every row length they serve, 0 never takes them); the results do not depend on it.  GPBC_ROWS_TABLE_MIN governs G1 only.
size_t rows_g2_table_min() {
    const char *e = getenv("GPBC_ROWS_G2_TABLE_MIN");
    if (!e || !*e) return ROWS_G2_TABLE_MIN;
    const unsigned long long v = strtoull(e, nullptr, 10);
    return v ? (size_t)v : ~(size_t)0;
}
