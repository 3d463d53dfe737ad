// Host build of the G2 row lane functions of csrc/rows29_g2.hip.hpp with -DGPBC_BOUNDS (every field element carries data-independent
// magnitude bounds, every product asserts that its int64 columns cannot overflow; abort() on violation): build (a), build (b) and the
// evaluation — the psi step on the accumulator included —, run lane by lane as the kernels of csrc/gpbc_rows_g2.hip run them.  A
// verification harness for tests/ only (tests/rows_g2_harness.py builds and loads it); never loaded by the product path.
//
// build: g++ -O2 -pthread -std=c++17 -DGPBC_BOUNDS -shared -fPIC -o tools/libgpbc_rows_g2_check.so tools/rows_g2_check.cpp
#ifndef GPBC_BOUNDS
#define GPBC_BOUNDS
#endif
#include <cstring>
#include "../gopairingbasedcryptography_amd/csrc/rows29_g2.hip.hpp"

using namespace gpbc;

static AffP<F2> ld_g2(const uint8_t *p) { return AffP<F2>{f2_load(p), f2_load(p + 64), bytes_all_zero(p, 32)}; }
static void st_g2(uint8_t *p, const AffP<F2> &r) { f2_store(p, r.x); f2_store(p + 64, r.y); }
static bool rows_aligned(const void *p) { return ((uintptr_t)p & 255) == 0; }
constexpr size_t BASE_DWORDS = (size_t)ROWS_G2_ENTRIES * ROWS_G2_ENTRY_DWORDS, WB_DWORDS = (size_t)ROWS_G2_WINDOWS * ROWS_G2_ENTRY_DWORDS;

extern "C" {

// [windows, digits, bytes of table per base, ROWS_G2_TABLE_MIN, ROWS_G2_PASS_OUTPUTS, ROWS_G2_TABLE_CAP, bytes of window bases per base,
//  ROWS_G2_GROUP_BASES]
void rg_geometry(size_t *out) {
    out[0] = ROWS_G2_WINDOWS; out[1] = ROWS_G2_DIGITS; out[2] = ROWS_G2_TABLE_BYTES; out[3] = ROWS_G2_TABLE_MIN; out[4] = ROWS_G2_PASS_OUTPUTS;
    out[5] = ROWS_G2_TABLE_CAP; out[6] = ROWS_G2_WB_BYTES; out[7] = ROWS_G2_GROUP_BASES;
}
size_t rg_pass_bases(size_t nbase, size_t m) { return m ? rows_g2_pass_bases(nbase, m) : 0; }

// build (a), one lane per base: wb = nbase x 4 352 bytes of window bases, 256-byte aligned; inf = nbase flags
int rg_build_a(const uint8_t *B, size_t nbase, int32_t *wb, uint8_t *inf) {
    if (!B || !wb || !inf || !rows_aligned(wb)) return -1;
    for (size_t j = 0; j < nbase; j++) rows_g2_build_a_lane(ld_g2(B + 128 * j), wb + j * WB_DWORDS, inf + j);
    return 0;
}
// build (b), one lane per (base, window), in the kernel's lane order: table = nbase x 65 280 bytes, 256-byte aligned
int rg_build_b(const int32_t *wb, int32_t *table, const uint8_t *inf, size_t nbase) {
    if (!wb || !table || !inf || !rows_aligned(wb) || !rows_aligned(table)) return -1;
    for (size_t q = 0; q < nbase * ROWS_G2_WINDOWS; q++)
        rows_g2_build_b_lane(wb + (q / ROWS_G2_WINDOWS) * WB_DWORDS, table + (q / ROWS_G2_WINDOWS) * BASE_DWORDS, inf + q / ROWS_G2_WINDOWS, (int)(q % ROWS_G2_WINDOWS));
    return 0;
}
// evaluation, one lane per output: out[j m + i] = [K[j m + i]] base_j; returns how many scalars had a quarter beyond the 17 windows (0)
int rg_eval(const int32_t *table, const uint8_t *inf, size_t nbase, size_t m, const uint8_t *K, uint8_t *out) {
    if (!table || !inf || !K || !out || !m || !rows_aligned(table)) return -1;
    int wide_count = 0;
    for (size_t i = 0; i < nbase * m; i++) {
        uint32_t k[8]; memcpy(k, K + 32 * i, 32);
        JacP<F2> acc;
        bool wide = false;
        rows_g2_eval_lane(acc, table + (i / m) * BASE_DWORDS, inf[i / m] != 0, k, &wide);
        wide_count += wide ? 1 : 0;
        AffP<F2> r;
        jac_to_affine(r, acc);
        st_g2(out + 128 * i, r);
    }
    return wide_count;
}
// the evaluation's walk on GIVEN splits, the rows of rg_gls_split: [k0, k1, k2, k3 (3 x u32 each), neg0 .. neg3] as 16 u32 per output;
// out[j m + i] = (sum +-k_i mu^i) base_j over the low 68 bits of the quarters
int rg_eval_split(const int32_t *table, const uint8_t *inf, size_t nbase, size_t m, const uint32_t *S, uint8_t *out) {
    if (!table || !inf || !S || !out || !m || !rows_aligned(table)) return -1;
    for (size_t i = 0; i < nbase * m; i++) {
        GlsSplit s;
        for (int q = 0; q < 4; q++) {
            for (int t = 0; t < 3; t++) s.k[q][t] = S[16 * i + 3 * q + t];
            s.neg[q] = S[16 * i + 12 + q] != 0;
        }
        JacP<F2> acc;
        rows_g2_eval_split(acc, table + (i / m) * BASE_DWORDS, inf[i / m] != 0, s);
        AffP<F2> r;
        jac_to_affine(r, acc);
        st_g2(out + 128 * i, r);
    }
    return 0;
}
// the split itself, in the same rows
void rg_gls_split(const uint8_t *K, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        uint32_t k[8]; memcpy(k, K + 32 * i, 32);
        GlsSplit s; gls_split(s, k);
        for (int q = 0; q < 4; q++) {
            for (int t = 0; t < 3; t++) out[16 * i + 3 * q + t] = s.k[q][t];
            out[16 * i + 12 + q] = s.neg[q];
        }
    }
}
// worst-case figures of this thread since it started: [max |int64 column|, max limb bound, max value bound (units of p), #products,
// #norms, #fe_mul2, #reduces]
void rg_stats(double *out) {
    BoundStats &s = bound_stats();
    out[0] = s.max_col; out[1] = s.max_limb; out[2] = s.max_vb; out[3] = (double)s.muls; out[4] = (double)s.norms; out[5] = (double)s.muls2; out[6] = (double)s.reduces;
}

}  // extern "C"
