// libgpbc_bn254.so, one of the units listed in _build.py: the elementwise group law — G1 / G2 addition, subtraction and doubling of affine points
// (csrc/group29.hip.hpp) with their C-ABI entries (include/gpbc_bn254.h).  gfx950 only.
#include "gpbc_common.hpp"
#include "group29.hip.hpp"

template <class F, int OP> __device__ __forceinline__ void group_kernel(const uint8_t *a, const uint8_t *b, size_t b_step, uint8_t *out, size_t n) {
    constexpr int K = group_k<F>();
    const size_t T = (n + K - 1) / K, t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= T) return;
    group_op_lane<F, K, OP>(a, b, b_step, out, n, t, T);
}
// (no __restrict__: out may be a, or b)
GPBC_KERNEL_G1 k_g1_add(const uint8_t *a, const uint8_t *b, size_t b_step, uint8_t *out, size_t n) { group_kernel<Fe, GROUP_ADD>(a, b, b_step, out, n); }
GPBC_KERNEL_G1 k_g1_sub(const uint8_t *a, const uint8_t *b, size_t b_step, uint8_t *out, size_t n) { group_kernel<Fe, GROUP_SUB>(a, b, b_step, out, n); }
GPBC_KERNEL_G1 k_g1_dbl(const uint8_t *a, const uint8_t *b, size_t b_step, uint8_t *out, size_t n) { group_kernel<Fe, GROUP_DBL>(a, b, b_step, out, n); }
GPBC_KERNEL k_g2_add(const uint8_t *a, const uint8_t *b, size_t b_step, uint8_t *out, size_t n) { group_kernel<F2, GROUP_ADD>(a, b, b_step, out, n); }
GPBC_KERNEL k_g2_sub(const uint8_t *a, const uint8_t *b, size_t b_step, uint8_t *out, size_t n) { group_kernel<F2, GROUP_SUB>(a, b, b_step, out, n); }
GPBC_KERNEL k_g2_dbl(const uint8_t *a, const uint8_t *b, size_t b_step, uint8_t *out, size_t n) { group_kernel<F2, GROUP_DBL>(a, b, b_step, out, n); }

extern "C" {

static int group_dev(bool g2, int op, const void *d_a, const void *d_b, size_t nb, size_t n, void *d_out, void *stream) {
    if (!n) return GPBC_OK;
    if (!d_a || !d_out || (op != GROUP_DBL && !d_b)) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    if (op != GROUP_DBL) TRY(nb_one_or_n(nb, n));
    TRY(bind_device());
    const hipStream_t st = (hipStream_t)stream;
    const uint8_t *a = (const uint8_t *)d_a, *b = op == GROUP_DBL ? a : (const uint8_t *)d_b;
    uint8_t *o = (uint8_t *)d_out;
    const size_t step = op != GROUP_DBL && nb == n ? (g2 ? GPBC_G2_BYTES : GPBC_G1_BYTES) : 0;
    const size_t K = g2 ? GROUP_K_G2 : GROUP_K_G1;
    const unsigned grid = grid_for((n + K - 1) / K);
    switch (op + (g2 ? 3 : 0)) {
        case 0: return GPBC_LAUNCH(k_g1_add, grid, BLOCK, st, a, b, step, o, n);
        case 1: return GPBC_LAUNCH(k_g1_sub, grid, BLOCK, st, a, b, step, o, n);
        case 2: return GPBC_LAUNCH(k_g1_dbl, grid, BLOCK, st, a, b, step, o, n);
        case 3: return GPBC_LAUNCH(k_g2_add, grid, BLOCK, st, a, b, step, o, n);
        case 4: return GPBC_LAUNCH(k_g2_sub, grid, BLOCK, st, a, b, step, o, n);
        default: return GPBC_LAUNCH(k_g2_dbl, grid, BLOCK, st, a, b, step, o, n);
    }
}
// Host-pointer entries: [0, n) sharded over the bound devices like the GT binary operations (a few microseconds of kernel per
// thousand elements, so a shard needs many of them to pay for its thread and transfers); calls of up to LANE_CALL_MAX_UNITS
// elements run on a call lane of their own (pinned block in and out, the lane's stream).  Not combined: a single Add costs a
// few microseconds on the host core, far less than any launch — it stays with gnark.
constexpr size_t GROUP_SHARD_MIN = 4 * 4096;
static int group_host(bool g2, int op, const void *a, const void *b, size_t nb, size_t n, void *out) {
    if (!n) return GPBC_OK;
    if (!a || !out || (op != GROUP_DBL && !b)) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    if (op != GROUP_DBL) TRY(nb_one_or_n(nb, n));
    const size_t pt = g2 ? GPBC_G2_BYTES : GPBC_G1_BYTES;
    const bool one = op != GROUP_DBL && nb == 1;
    HostCall c = HostCall().input(a, pt);
    if (op != GROUP_DBL) c.input(b, pt, one);
    return host_call_sharded(n, GROUP_SHARD_MIN, c.output(out, pt), HostRoute{CALL_KINDS, nullptr, 0, LANE_CALL_MAX_UNITS},
                             [=](const DevCols &d, size_t m, hipStream_t st) { return group_dev(g2, op, d.in[0], d.in[1], one ? 1 : m, m, d.out[0], st); });
}
int gpbc_g1_add_batch(const void *a, const void *b, size_t nb, size_t n, void *o) { return group_host(false, GROUP_ADD, a, b, nb, n, o); }
int gpbc_g1_sub_batch(const void *a, const void *b, size_t nb, size_t n, void *o) { return group_host(false, GROUP_SUB, a, b, nb, n, o); }
int gpbc_g1_double_batch(const void *a, size_t n, void *o) { return group_host(false, GROUP_DBL, a, nullptr, n, n, o); }
int gpbc_g2_add_batch(const void *a, const void *b, size_t nb, size_t n, void *o) { return group_host(true, GROUP_ADD, a, b, nb, n, o); }
int gpbc_g2_sub_batch(const void *a, const void *b, size_t nb, size_t n, void *o) { return group_host(true, GROUP_SUB, a, b, nb, n, o); }
int gpbc_g2_double_batch(const void *a, size_t n, void *o) { return group_host(true, GROUP_DBL, a, nullptr, n, n, o); }
int gpbc_g1_add_batch_dev(const void *a, const void *b, size_t nb, size_t n, void *o, void *st) { return group_dev(false, GROUP_ADD, a, b, nb, n, o, st); }
int gpbc_g1_sub_batch_dev(const void *a, const void *b, size_t nb, size_t n, void *o, void *st) { return group_dev(false, GROUP_SUB, a, b, nb, n, o, st); }
int gpbc_g1_double_batch_dev(const void *a, size_t n, void *o, void *st) { return group_dev(false, GROUP_DBL, a, nullptr, n, n, o, st); }
int gpbc_g2_add_batch_dev(const void *a, const void *b, size_t nb, size_t n, void *o, void *st) { return group_dev(true, GROUP_ADD, a, b, nb, n, o, st); }
int gpbc_g2_sub_batch_dev(const void *a, const void *b, size_t nb, size_t n, void *o, void *st) { return group_dev(true, GROUP_SUB, a, b, nb, n, o, st); }
int gpbc_g2_double_batch_dev(const void *a, size_t n, void *o, void *st) { return group_dev(true, GROUP_DBL, a, nullptr, n, n, o, st); }

}  // extern "C"
