// The LDS memory policy of the latency form (wide29.hip.hpp): slot loads / stores and struct WideLds with its one-limb-per-lane
// operations.  A header of its own so that tools/check_limb_ops.hip can run exactly this code on crafted slot contents without the
// kernels of gpbc_pairing.hip.  Device only.
#ifndef GPBC_WIDE_LDS29_HIP_HPP
#define GPBC_WIDE_LDS29_HIP_HPP
#include "wide29.hip.hpp"

using namespace gpbc;    // as gpbc_common.hpp has it: this code stands outside the namespace, where gpbc_pairing.hip defined it

typedef int32_t w128 __attribute__((ext_vector_type(4)));
// one slot = 96 bytes: a0 in three 128-bit words (nine limbs + padding), a1 in the next three — either half can be read or written alone
__device__ __forceinline__ Fe wide_half_load(const w128 *mem, int slot, int h) {
    const w128 t0 = mem[slot * 6 + 3 * h], t1 = mem[slot * 6 + 3 * h + 1], t2 = mem[slot * 6 + 3 * h + 2];
    Fe r;
    r.v[0] = t0.x; r.v[1] = t0.y; r.v[2] = t0.z; r.v[3] = t0.w; r.v[4] = t1.x; r.v[5] = t1.y; r.v[6] = t1.z; r.v[7] = t1.w; r.v[8] = t2.x;
    return r;
}
__device__ __forceinline__ void wide_half_store(w128 *mem, int slot, int h, const Fe &v) {
    mem[slot * 6 + 3 * h] = w128{v.v[0], v.v[1], v.v[2], v.v[3]};
    mem[slot * 6 + 3 * h + 1] = w128{v.v[4], v.v[5], v.v[6], v.v[7]};
    mem[slot * 6 + 3 * h + 2] = w128{v.v[8], 0, 0, 0};
}
__device__ __forceinline__ F2 wide_slot_load(const w128 *mem, int slot) { return F2{wide_half_load(mem, slot, 0), wide_half_load(mem, slot, 1)}; }
__device__ __forceinline__ void wide_slot_store(w128 *mem, int slot, const F2 &v) { wide_half_store(mem, slot, 0, v.a0); wide_half_store(mem, slot, 1, v.a1); }
// The phases of ONE WAVE: its LDS instructions execute in program order, so a phase's stores are visible to the next phase's loads
// of any lane of the same wave; the fence / wave barrier only keeps the compiler from moving LDS accesses across the phase boundary.
// A workgroup of the exponentiation / product kernels may bring a HELPER wave (128 threads instead of 64): it sits out every phase
// except the product phase of wide_mul (run2), where the 72 halves of the 36 F2 products go to 72 lanes of the two waves instead of
// 36 whole products to one — a lone wave issues one MAD per ~9 cycles, so that phase is halved.  Calls of more than 1 024 elements
// come without it (two waves per element would need a second round of the chip).
struct WideLds {
    w128 *mem;
    int lane;                                                // lane number inside the wave
    int helper = 0, n_waves = 1;                             // helper: this wave only takes part in run2 phases
    __device__ __forceinline__ int waves() const { return n_waves; }
    // limb-parallel phases (wide29.hip.hpp: wide_cyclo_out_limbs): lane = component * NL + limb
    static constexpr bool LIMB_PARALLEL = true;
    __device__ __forceinline__ int comp() const { return lane / NL; }
    __device__ __forceinline__ int limb() const { return lane % NL; }
    __device__ __forceinline__ int32_t p_limb() const {      // this lane's limb of p
        constexpr int32_t P[NL] = F29_P;
        const int i = limb();
        int32_t r = P[0];
#pragma unroll
        for (int j = 1; j < NL; j++) r = i == j ? P[j] : r;
        return r;
    }
    __device__ __forceinline__ int32_t ldw(int slot, int h, int i) const { return reinterpret_cast<const int32_t *>(mem)[(slot * 6 + 3 * h) * 4 + i]; }
    __device__ __forceinline__ void stw(int slot, int h, int i, int32_t v) const { reinterpret_cast<int32_t *>(mem)[(slot * 6 + 3 * h) * 4 + i] = v; }
    __device__ __forceinline__ static int32_t below(int32_t v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xF, 0xF, true); }   // the value of lane - 1 (wave_shr:1)
    __device__ __forceinline__ int32_t from_top(int32_t v) const { return __builtin_amdgcn_ds_bpermute((comp() * NL + NL - 1) * 4, v); }   // ... of the lane that holds the component's top limb
    __device__ __forceinline__ F2 ld(int slot) const { return wide_slot_load(mem, slot); }
    __device__ __forceinline__ void st(int slot, const F2 &v) const { wide_slot_store(mem, slot, v); }
    __device__ __forceinline__ Fe ldh(int slot, int h) const { return wide_half_load(mem, slot, h); }
    __device__ __forceinline__ void sth(int slot, int h, const Fe &v) const { wide_half_store(mem, slot, h, v); }
    template <class B> __device__ __forceinline__ void run(int n, B &&body) const {
        if (!helper && lane < n) body(lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // a phase of BOTH waves (n <= 128 lanes; only where waves() == 2): workgroup barriers on both sides — every wave of the workgroup
    // walks the same (uniform) control flow, so both reach them
    // one-limb-per-lane operations of the linear phases (wide29.hip.hpp "linear phases"): lane = component * NL + limb
    struct LimbOps {
        using V = int32_t;
        const WideLds &m;
        int i;
        int32_t low, carry_in, p_i;
        __device__ __forceinline__ explicit LimbOps(const WideLds &w) : m(w), i(w.limb()), low(w.limb() == NL - 1 ? -1 : LMASK), carry_in(w.limb() == 0 ? 0 : -1), p_i(w.p_limb()) {}
        __device__ __forceinline__ V ld(int slot, int h) const { return m.ldw(slot, h, i); }
        __device__ __forceinline__ void st(int slot, int h, V v) const { m.stw(slot, h, i, v); }
        __device__ __forceinline__ static V add(V a, V b) { return a + b; }
        __device__ __forceinline__ static V sub(V a, V b) { return a - b; }
        __device__ __forceinline__ static V dbl(V a) { return a + a; }
        __device__ __forceinline__ static V neg(V a) { return -a; }
        __device__ __forceinline__ static V sel(bool c, V a, V b) { return c ? a : b; }
        __device__ __forceinline__ V norm(V v) const { return (v & low) + ((below(v) >> LB) & carry_in); }                  // fe_norm
        __device__ __forceinline__ V halve(V v) const {                                                                    // fe_halve
            const int32_t odd = -(__builtin_amdgcn_ds_bpermute(m.comp() * NL * 4, v) & 1);                                   // parity of the value = parity of limb 0
            const int32_t t = v + (p_i & odd);
            const int32_t up = __builtin_amdgcn_update_dpp(0, t, 0x130, 0xF, 0xF, true);                                     // the limb above (wave_shl:1)
            return (t >> 1) + (i == NL - 1 ? 0 : (up & 1) << (LB - 1));
        }
    };
    template <class B> __device__ __forceinline__ void limbs(int n_comp, B &&body) const {
        run(n_comp * NL, [&](int) { LimbOps o(*this); body(o, comp()); });
    }
    __device__ __forceinline__ void sync_waves() const { if (n_waves == 2) __syncthreads(); }    // before control flow that depends on LDS contents
    template <class B> __device__ __forceinline__ void run2(int n, B &&body) const {
        __syncthreads();
        const int l = helper * 64 + lane;
        if (l < n) body(l);
        __syncthreads();
    }
};
#endif
