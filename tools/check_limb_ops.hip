// Device-side run of the data-dependent field routines (csrc/fe29.hip.hpp) and of their one-limb-per-lane forms (csrc/wide_lds29.hip.hpp:
// WideLds::LimbOps; csrc/wide29.hip.hpp: the LIMB_PARALLEL branches of wide_recombine and wide_cyclo_out_limbs) on raw limbs and crafted
// LDS slot contents.  The host interval harness runs the Fe-level branch and has no DPP, no ds_bpermute, no device rintf and no F29_KP in
// device memory; whole pairings reach this code only with small multipliers k and positive carries.  This program judges nothing: it
// reads records, runs them, writes raw int32 limbs back; tests/test_limb_ops_gpu.py builds the records from tests/limb_cases.py and
// compares.  It instantiates no Miller loop and no final exponentiation.
//   build: hipcc -O3 --offload-arch=gfx950 -std=c++17 -I <csrc> tools/check_limb_ops.hip        run: check_limb_ops <in> <out>
// Input (int32, little-endian): magic, nA, nB, nC, nD1, nD2, then the records of each section; output: the results in the same order.
//   A  op, a[9], b[9]                            -> out[9], flag       one case per LANE (op numbers of hc_fe_primitive)
//   B  op, n_comp, a[7][9], b[7][9]              -> out[7][9]          one case per wavefront: WideLds::limbs(n_comp, ...)
//   C  alias, prod[9][2][9], a[6][2][9]          -> dst[6][2][9]       wide_cyclo_out_limbs<true> then <false>; alias: dst is a
//   D  op, A[6][2][9], B[6][2][9]                -> limb form [6][2][9], Fe form [6][2][9]     0 wide_mul, 1 wide_sqr, 2 wide_mul_line
//      (the line: B's first three slots), 3 wide_cyclo_sqr; the nD1 records run on 64 threads, the nD2 (wide_mul only) on 128: with the helper wave
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "wide_lds29.hip.hpp"
using namespace gpbc;
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

constexpr int MAGIC = 0x4c4d4231;
constexpr int REC_A = 1 + 2 * NL, OUT_A = NL + 1;
constexpr int MAX_COMP = 7, REC_B = 2 + 2 * MAX_COMP * NL, OUT_B = MAX_COMP * NL;
constexpr int VAL = 6 * 2 * NL;                               // one Fp12 value as raw limbs: slot, half, limb
constexpr int REC_C = 1 + 9 * 2 * NL + VAL, OUT_C = VAL;
constexpr int REC_D = 1 + 2 * VAL, OUT_D = 2 * VAL;
// the Fe-level branch of the wide operations, on the device
struct WideLdsFe : WideLds { static constexpr bool LIMB_PARALLEL = false; };

__device__ __forceinline__ Fe fe_raw(const int32_t *w) {
    Fe r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.v[i] = w[i];
    return r;
}
__device__ __forceinline__ void fe_raw_store(int32_t *w, const Fe &r) {
#pragma unroll
    for (int i = 0; i < NL; i++) w[i] = r.v[i];
}

__global__ void __launch_bounds__(64) k_fe_ops(const int32_t *__restrict__ in, int32_t *__restrict__ out, int n) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    const int32_t *rec = in + (size_t)t * REC_A;
    const Fe a = fe_raw(rec + 1), b = fe_raw(rec + 1 + NL);
    Fe r = fe_zero();
    int flag = 0;
    switch (rec[0]) {
    case 0: r = fe_norm(a); break;
    case 1: r = fe_mul8_norm(a); break;
    case 2: r = fe_halve(a); break;
    case 3: r = fe_reduce(a); break;
    case 4: r = fe_reduce_arith(a); break;
    case 5: r = fe_reduce_arith_norm(a); break;
    case 6: r = fe_cyclo_out(a, b); break;
    case 7: r = fe_canonical(a); break;
    case 8: flag = fe_is_zero(a) ? 1 : 0; break;
    default: flag = -1; break;
    }
    fe_raw_store(out + (size_t)t * OUT_A, r);
    out[(size_t)t * OUT_A + NL] = flag;
}

// component c: operand a in half c of slots 0.., b in slots 4.., result in slots 8..
__global__ void __launch_bounds__(64) k_limb_ops(const int32_t *__restrict__ in, int32_t *__restrict__ out, int n) {
    __shared__ w128 w_mem[12 * 6];
    if ((int)blockIdx.x >= n) return;
    const int32_t *rec = in + (size_t)blockIdx.x * REC_B;
    const int op = rec[0], n_comp = rec[1] < 1 ? 1 : rec[1] > MAX_COMP ? MAX_COMP : rec[1];
    const WideLds m{w_mem, (int)threadIdx.x};
    m.run(n_comp, [&](int c) {
        m.sth(c >> 1, c & 1, fe_raw(rec + 2 + c * NL));
        m.sth(4 + (c >> 1), c & 1, fe_raw(rec + 2 + (MAX_COMP + c) * NL));
    });
    m.limbs(n_comp, [&](auto &o, int c) {
        const auto a = o.ld(c >> 1, c & 1), b = o.ld(4 + (c >> 1), c & 1);
        auto r = a;
        switch (op) {
        case 0: r = o.norm(a); break;
        case 1: r = o.halve(a); break;
        case 2: r = o.add(a, b); break;
        case 3: r = o.sub(a, b); break;
        case 4: r = o.dbl(a); break;
        case 5: r = o.neg(a); break;
        case 6: r = o.sel(c & 1, a, b); break;
        case 7: r = o.norm(o.sub(a, o.add(o.dbl(b), b))); break;
        default: r = o.norm(o.halve(o.norm(o.add(a, b)))); break;
        }
        o.st(8 + (c >> 1), c & 1, r);
    });
    m.run(n_comp, [&](int c) { fe_raw_store(out + (size_t)blockIdx.x * OUT_B + c * NL, m.ldh(8 + (c >> 1), c & 1)); });
}

__global__ void __launch_bounds__(64) k_cyclo_out(const int32_t *__restrict__ in, int32_t *__restrict__ out, int n) {
    __shared__ w128 w_mem[W_SLOTS * 6];
    if ((int)blockIdx.x >= n) return;
    const int32_t *rec = in + (size_t)blockIdx.x * REC_C;
    const int a = wv(0), dst = rec[0] ? wv(0) : wv(1);
    const WideLds m{w_mem, (int)threadIdx.x};
    m.run(30, [&](int L) {
        if (L < 18) m.sth(W_PROD + (L >> 1), L & 1, fe_raw(rec + 1 + L * NL));
        else m.sth(a + ((L - 18) >> 1), L & 1, fe_raw(rec + 1 + L * NL));
    });
    wide_cyclo_out_limbs<true>(m, dst, a);
    wide_cyclo_out_limbs<false>(m, dst, a);
    m.run(12, [&](int L) { fe_raw_store(out + (size_t)blockIdx.x * OUT_C + L * NL, m.ldh(dst + (L >> 1), L & 1)); });
}

template <class M> __device__ __forceinline__ void wide_case(const M &m, int op, const int32_t *rec, int32_t *out) {
    constexpr int A = wv(0), Bv = wv(1), D = wv(2);
    m.run(24, [&](int L) { m.sth((L >> 1), L & 1, fe_raw(rec + 1 + L * NL)); });            // values 0 and 1 are slots 0..11
    if (op == 0) wide_mul(m, D, A, Bv);
    else if (op == 1) wide_sqr(m, D, A);
    else if (op == 2) wide_mul_line(m, D, A, Bv);
    else wide_cyclo_sqr(m, D, A);
    m.run(12, [&](int L) { fe_raw_store(out + L * NL, m.ldh(D + (L >> 1), L & 1)); });
}
__global__ void __launch_bounds__(128) k_wide_ops(const int32_t *__restrict__ in, int32_t *__restrict__ out, int n) {
    __shared__ w128 w_mem[W_SLOTS * 6];
    if ((int)blockIdx.x >= n) return;
    const int32_t *rec = in + (size_t)blockIdx.x * REC_D;
    int32_t *o = out + (size_t)blockIdx.x * OUT_D;
    const int waves = (int)(blockDim.x >> 6), op = waves == 2 ? 0 : rec[0];                 // the helper wave only knows wide_mul's product phase
    const WideLds m{w_mem, (int)(threadIdx.x & 63), (int)(threadIdx.x >> 6), waves};
    WideLdsFe f;
    f.mem = w_mem; f.lane = m.lane; f.helper = m.helper; f.n_waves = m.n_waves;
    wide_case(m, op, rec, o);
    __syncthreads();                                                                        // (uniform: every wave of the workgroup comes here)
    wide_case(f, op, rec, o + VAL);
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <input> <output>\n", argv[0]); return 2; }
    FILE *fi = fopen(argv[1], "rb");
    if (!fi) { perror(argv[1]); return 2; }
    int32_t head[6];
    if (fread(head, 4, 6, fi) != 6 || head[0] != MAGIC) { fprintf(stderr, "bad header\n"); return 2; }
    const int rec[5] = {REC_A, REC_B, REC_C, REC_D, REC_D}, res[5] = {OUT_A, OUT_B, OUT_C, OUT_D, OUT_D};
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) { perror(argv[2]); return 2; }
    for (int s = 0; s < 5; s++) {
        const int n = head[1 + s];
        if (n < 0 || n > (1 << 20)) { fprintf(stderr, "bad count\n"); return 2; }
        if (n == 0) continue;
        std::vector<int32_t> h((size_t)n * rec[s]), r((size_t)n * res[s], 0);
        if (fread(h.data(), 4, h.size(), fi) != h.size()) { fprintf(stderr, "short input, section %d\n", s); return 2; }
        int32_t *din, *dout;
        CHECK(hipMalloc(&din, h.size() * 4)); CHECK(hipMalloc(&dout, r.size() * 4));
        CHECK(hipMemcpy(din, h.data(), h.size() * 4, hipMemcpyHostToDevice));
        CHECK(hipMemset(dout, 0, r.size() * 4));
        if (s == 0) k_fe_ops<<<(n + 63) / 64, 64>>>(din, dout, n);
        if (s == 1) k_limb_ops<<<n, 64>>>(din, dout, n);
        if (s == 2) k_cyclo_out<<<n, 64>>>(din, dout, n);
        if (s == 3) k_wide_ops<<<n, 64>>>(din, dout, n);
        if (s == 4) k_wide_ops<<<n, 128>>>(din, dout, n);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(r.data(), dout, r.size() * 4, hipMemcpyDeviceToHost));
        CHECK(hipFree(din)); CHECK(hipFree(dout));
        if (fwrite(r.data(), 4, r.size(), fo) != r.size()) { perror("write"); return 2; }
        printf("section %c: %d cases\n", "ABCDE"[s], n);
    }
    fclose(fi);
    if (fclose(fo)) { perror("close"); return 2; }
    return 0;
}
