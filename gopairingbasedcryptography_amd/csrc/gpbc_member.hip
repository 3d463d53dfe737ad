// libgpbc_bn254.so, the twelfth unit (_build.MEMBER_SOURCES): membership of in-memory G1, G2 and GT elements (csrc/member29.hip.hpp) with the
// C-ABI entries of include/gpbc_bn254_member.h.  gfx950 only.
// A unit of its own, and not beside g2_in_subgroup29's callers in gpbc_wire.hip and the lane-pair Fp12 kernels in gpbc_pairing.hip, where
// the lane bodies come from: with k_gt_is_in_subgroup in gpbc_pairing.hip the compiler scheduled f12p_expt_to and k_final_exp differently
// (the non-inlined x^u chain got one more caller), and the headline benchmark's three runs all came out below the parent's (0.2 % at the
// medians).  Here every older unit is the parent's source and compiles to the parent's code; the price is a second copy of
// f12p_expt_to, f12p_mul_to and g2_in_subgroup29 in the library.
#include "gpbc_common.hpp"
#include "member29.hip.hpp"
#include "../../include/gpbc_bn254_member.h"

// ---- points: one per lane, a verdict byte each and nothing else written
GPBC_KERNEL k_g1_is_on_curve(const uint8_t *__restrict__ pts, uint8_t *__restrict__ ok, size_t n) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    ok[i] = g1_member_on_curve(pts + i * GPBC_G1_BYTES) ? 1 : 0;
}
GPBC_KERNEL k_g2_is_on_curve(const uint8_t *__restrict__ pts, uint8_t *__restrict__ ok, size_t n) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    ok[i] = g2_member(pts + i * GPBC_G2_BYTES, false) ? 1 : 0;
}
GPBC_KERNEL k_g2_is_in_subgroup(const uint8_t *__restrict__ pts, uint8_t *__restrict__ ok, size_t n) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    ok[i] = g2_member(pts + i * GPBC_G2_BYTES, true) ? 1 : 0;
}
// ---- GT: one element per lane pair, the loader and the lane layout of k_final_exp / k_gt_exp (even lane C0, odd lane C1).  The pair past
// the last element returns together; nothing but ok[i] is written.
GPBC_KERNEL k_gt_is_in_subgroup(const uint8_t *__restrict__ gt, uint8_t *__restrict__ ok, size_t n) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x, i = lane >> 1;
    if (i >= n) return;
    PairDpp x{(bool)(lane & 1)};
    const bool good = gt_member_pair(x, gt + i * GPBC_GT_BYTES + (x.odd ? 192 : 0), false);
    if (!x.odd) ok[i] = good ? 1 : 0;
}

extern "C" {

int gpbc_member_version(void) { return 1; }

// kind 0 = G1 on the curve, 1 = G2 on the twist, 2 = G2 in the subgroup, 3 = GT in the subgroup.  ONE launch, no workspace.
static size_t member_row_bytes(int kind) { return kind == 0 ? GPBC_G1_BYTES : kind == 3 ? GPBC_GT_BYTES : GPBC_G2_BYTES; }
static int member_args(int kind, const void *in, size_t n, const void *ok_out) {
    if (!n) return GPBC_OK;
    TRY(call_limit("rows", n, 0x7fffffff));
    if (!in || !ok_out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    if ((uintptr_t)in & 3) return fail(GPBC_ERR_INVALID_ARG, "rows must be 4-byte aligned");
    if (ranges_overlap(in, n * member_row_bytes(kind), ok_out, n)) return fail(GPBC_ERR_INVALID_ARG, "ok_out overlaps the input");
    return GPBC_OK;
}
static int member_dev(int kind, const void *d_in, size_t n, uint8_t *d_ok_out, void *stream) {
    TRY(member_args(kind, d_in, n, d_ok_out));
    if (!n) return GPBC_OK;
    TRY(bind_device());
    hipStream_t st = (hipStream_t)stream;
    const uint8_t *in = (const uint8_t *)d_in;
    if (kind == 0) return GPBC_LAUNCH(k_g1_is_on_curve, grid_for(n), BLOCK, st, in, d_ok_out, n);
    if (kind == 1) return GPBC_LAUNCH(k_g2_is_on_curve, grid_for(n), BLOCK, st, in, d_ok_out, n);
    if (kind == 2) return GPBC_LAUNCH(k_g2_is_in_subgroup, grid_for(n), BLOCK, st, in, d_ok_out, n);
    return GPBC_LAUNCH(k_gt_is_in_subgroup, grid_for(2 * n), BLOCK, st, in, d_ok_out, n);
}
// the shared staging path on the calling thread's current device: not sharded, not combined
static int member_host(int kind, const void *in, size_t n, uint8_t *ok_out) {
    TRY(member_args(kind, in, n, ok_out));
    if (!n) return GPBC_OK;
    return host_call(n, HostCall().input(in, member_row_bytes(kind)).output(ok_out, 1), HostRoute{},
                     [=](const DevCols &d, size_t m, hipStream_t st) { return member_dev(kind, d.in[0], m, d.out[0], st); });
}
int gpbc_g1_is_on_curve(const void *p, size_t n, uint8_t *ok) { return member_host(0, p, n, ok); }
int gpbc_g2_is_on_curve(const void *p, size_t n, uint8_t *ok) { return member_host(1, p, n, ok); }
int gpbc_g2_is_in_subgroup(const void *p, size_t n, uint8_t *ok) { return member_host(2, p, n, ok); }
int gpbc_gt_is_in_subgroup(const void *g, size_t n, uint8_t *ok) { return member_host(3, g, n, ok); }
int gpbc_g1_is_on_curve_dev(const void *p, size_t n, uint8_t *ok, void *st) { return member_dev(0, p, n, ok, st); }
int gpbc_g2_is_on_curve_dev(const void *p, size_t n, uint8_t *ok, void *st) { return member_dev(1, p, n, ok, st); }
int gpbc_g2_is_in_subgroup_dev(const void *p, size_t n, uint8_t *ok, void *st) { return member_dev(2, p, n, ok, st); }
int gpbc_gt_is_in_subgroup_dev(const void *g, size_t n, uint8_t *ok, void *st) { return member_dev(3, g, n, ok, st); }

}  // extern "C"
