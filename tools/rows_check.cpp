// Host build of the row lane functions of csrc/rows29.hip.hpp with -DGPBC_BOUNDS (every field element carries data-independent
// magnitude bounds, every product asserts that its int64 columns cannot overflow; abort() on violation): build (a), build (b), the
// evaluation and the table-free row lane, run lane by lane as the kernels of csrc/gpbc_rows.hip run them.  A verification harness for
// tests/ only (tests/rows_harness.py builds and loads it); never loaded by the product path.
//
// build: g++ -O2 -pthread -std=c++17 -DGPBC_BOUNDS -shared -fPIC -o tools/libgpbc_rows_check.so tools/rows_check.cpp
#ifndef GPBC_BOUNDS
#define GPBC_BOUNDS
#endif
#include <cstring>
#include "../gopairingbasedcryptography_amd/csrc/rows29.hip.hpp"

using namespace gpbc;

static AffP<Fe> ld_g1(const uint8_t *p) { return AffP<Fe>{fe_load(p), fe_load(p + 32), bytes_all_zero(p, 16)}; }
static void st_g1(uint8_t *p, const AffP<Fe> &r) { fe_store(p, r.x); fe_store(p + 32, r.y); }
static AffP<F2> ld_g2(const uint8_t *p) { return AffP<F2>{f2_load(p), f2_load(p + 64), bytes_all_zero(p, 32)}; }
static void st_g2(uint8_t *p, const AffP<F2> &r) { f2_store(p, r.x); f2_store(p + 64, r.y); }
static bool rows_aligned(const void *p) { return ((uintptr_t)p & 127) == 0; }
constexpr size_t BASE_DWORDS = (size_t)ROWS_ENTRIES * ROWS_ENTRY_DWORDS, WB_DWORDS = (size_t)ROWS_WINDOWS * ROWS_ENTRY_DWORDS;

extern "C" {

// [windows, digits, bytes of table per base, ROWS_TABLE_MIN, ROWS_PASS_OUTPUTS, ROWS_TABLE_CAP, bytes of window bases per base, ROWS_GROUP_BASES]
void rc_geometry(size_t *out) {
    out[0] = ROWS_WINDOWS; out[1] = ROWS_DIGITS; out[2] = ROWS_TABLE_BYTES; out[3] = ROWS_TABLE_MIN; out[4] = ROWS_PASS_OUTPUTS; out[5] = ROWS_TABLE_CAP;
    out[6] = ROWS_WB_BYTES; out[7] = ROWS_GROUP_BASES;
}
size_t rc_pass_bases(size_t nbase, size_t m) { return m ? rows_pass_bases(nbase, m) : 0; }

// build (a), one lane per base: wb = nbase x 4 096 bytes of window bases, 128-byte aligned; inf = nbase flags
int rc_build_a(const uint8_t *B, size_t nbase, int32_t *wb, uint8_t *inf) {
    if (!B || !wb || !inf || !rows_aligned(wb)) return -1;
    for (size_t j = 0; j < nbase; j++) rows_build_a_lane(ld_g1(B + 64 * j), wb + j * WB_DWORDS, inf + j);
    return 0;
}
// build (b), one lane per (base, window), in the kernel's lane order: table = nbase x 61 440 bytes, 128-byte aligned
int rc_build_b(const int32_t *wb, int32_t *table, const uint8_t *inf, size_t nbase) {
    if (!wb || !table || !inf || !rows_aligned(wb) || !rows_aligned(table)) return -1;
    for (size_t q = 0; q < nbase * ROWS_WINDOWS; q++)
        rows_build_b_lane(wb + (q / ROWS_WINDOWS) * WB_DWORDS, table + (q / ROWS_WINDOWS) * BASE_DWORDS, inf + q / ROWS_WINDOWS, (int)(q % ROWS_WINDOWS));
    return 0;
}
// evaluation, one lane per output: out[j m + i] = [K[j m + i]] base_j; returns how many scalars had a half of more than 128 bits (0)
int rc_eval(const int32_t *table, const uint8_t *inf, size_t nbase, size_t m, const uint8_t *K, uint8_t *out) {
    if (!table || !inf || !K || !out || !m || !rows_aligned(table)) return -1;
    int wide_count = 0;
    for (size_t i = 0; i < nbase * m; i++) {
        uint32_t k[8]; memcpy(k, K + 32 * i, 32);
        JacP<Fe> acc;
        bool wide = false;
        rows_eval_lane(acc, table + (i / m) * BASE_DWORDS, inf[i / m] != 0, k, &wide);
        wide_count += wide ? 1 : 0;
        AffP<Fe> r;
        jac_to_affine(r, acc);
        st_g1(out + 64 * i, r);
    }
    return wide_count;
}
// the evaluation's walk on GIVEN splits, the rows of hc_glv_split: [k1 (5 x u32), k2 (5 x u32), neg1, neg2] as 12 u32 per output;
// out[j m + i] = (+-k1 +- k2 lambda) base_j over the low 128 bits of the halves
int rc_eval_split(const int32_t *table, const uint8_t *inf, size_t nbase, size_t m, const uint32_t *S, uint8_t *out) {
    if (!table || !inf || !S || !out || !m || !rows_aligned(table)) return -1;
    for (size_t i = 0; i < nbase * m; i++) {
        GlvSplit s;
        for (int t = 0; t < 5; t++) { s.k1[t] = S[12 * i + t]; s.k2[t] = S[12 * i + 5 + t]; }
        s.neg1 = S[12 * i + 10] != 0; s.neg2 = S[12 * i + 11] != 0;
        JacP<Fe> acc;
        rows_eval_split(acc, table + (i / m) * BASE_DWORDS, inf[i / m] != 0, s);
        AffP<Fe> r;
        jac_to_affine(r, acc);
        st_g1(out + 64 * i, r);
    }
    return 0;
}
// the split itself, in the same rows
void rc_glv_split(const uint8_t *K, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        uint32_t k[8]; memcpy(k, K + 32 * i, 32);
        GlvSplit s; glv_split(s, k);
        for (int t = 0; t < 5; t++) { out[12 * i + t] = s.k1[t]; out[12 * i + 5 + t] = s.k2[t]; }
        out[12 * i + 10] = s.neg1; out[12 * i + 11] = s.neg2;
    }
}
// the table-free row lane: lane i on base i / m
int rc_rows_free(int is_g2, const uint8_t *B, size_t nbase, size_t m, const uint8_t *K, uint8_t *out) {
    if (!B || !K || !out || !m) return -1;
    for (size_t i = 0; i < nbase * m; i++) {
        uint32_t k[8]; memcpy(k, K + 32 * i, 32);
        if (is_g2) {
            alignas(128) int32_t tab[glv_table_dwords<F2>()];
            AffP<F2> r;
            rows_free_lane<F2>(r, ld_g2(B + 128 * (i / m)), k, tab);
            st_g2(out + 128 * i, r);
        } else {
            alignas(128) int32_t tab[glv_table_dwords<Fe>()];
            AffP<Fe> r;
            rows_free_lane<Fe>(r, ld_g1(B + 64 * (i / m)), k, tab);
            st_g1(out + 64 * i, r);
        }
    }
    return 0;
}
// worst-case figures of this thread since it started: [max |int64 column|, max limb bound, max value bound (units of p), #products,
// #norms, #fe_mul2, #reduces]
void rc_stats(double *out) {
    BoundStats &s = bound_stats();
    out[0] = s.max_col; out[1] = s.max_limb; out[2] = s.max_vb; out[3] = (double)s.muls; out[4] = (double)s.norms; out[5] = (double)s.muls2; out[6] = (double)s.reduces;
}

}  // extern "C"
