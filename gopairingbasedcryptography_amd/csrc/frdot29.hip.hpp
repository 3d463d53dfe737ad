// Segmented inner products in Fr for gfx950: out[s] = sum_{i in [seg_off[s], seg_off[s+1])} a[i] b[i] mod r, with one b per element,
// one list of b for segments of one length, or no b at all (the plain sum) — the sums  sum rho_i  and  sum w_i share_i  that a batch
// verifier and the planners' own checks need (signature/bls01_signature/bls_signature.go:71-89, zss04_signature.go:300-340,
// bb04_signature.go:262-295 verify one signature each; the weighted equation over many of them is built from these sums).  The third shape
// on csrc/segred29.hip.hpp, beside the GT multi-exponentiation and the G1 / G2 multi-scalar multiplication: the same cut, level walk and
// workspace plan; the fold levels are plain sums.  The kernel (k_fr_dot_segments in csrc/gpbc_fr.hip) and the host interval harness
// (tools/bounds_check.cpp: hc_fr_dot_segments) run the functions below.
//
// L neighbouring lanes per piece, L = 64 (a whole wavefront) down to 8, chosen per launch from the mean piece length (fr_dot_lanes: the
// smallest L that leaves a lane at most two elements of a mean piece, so that 2^16 segments of 16 elements are 8192 wavefronts of eight
// pieces and not 65536 wavefronts with 48 idle lanes — measured: 0.135 ms before, DESIGN.md has the figure after).  The kernel reads 64
// (or 32) bytes per element and does one product, so what matters is that the loads of a wavefront coalesce: lane l of a piece takes
// the elements a + l, a + l + L, ... of [a, b), so one load instruction covers L x 32 consecutive bytes per piece — 2 KiB per operand
// at L = 64, and at least 256 bytes, two whole 128-byte lines, at L = 8, with the pieces of neighbouring segments next to each other
// (a lane walking a piece of its own would put the 64 loads a whole piece apart, 64 different lines per instruction).  A lane's 32
// bytes are fetched as two 128-bit loads when the operand's base is 16-byte aligned, as eight dwords otherwise (by address, uniform
// over the launch).  No LDS: the only exchange is the fold of the L partial sums at the end, log2(L) butterfly steps through
// ds_bpermute (__shfl_xor), which uses the LDS crossbar but no LDS memory.
// The trip count is the WAVEFRONT's: the largest ceil(len / 2L) of its pieces, rounds of two elements per lane.  A lane whose element
// lies past the end of its piece — or whose piece is shorter than its neighbour's, or does not exist — multiplies zeros instead of
// leaving the loop, so no lane of a wavefront ever runs fewer rounds than another and the fold is reached by all 64 lanes together
// (csrc/gmsm29.hip.hpp records wrong sums on gfx950 for lanes with G and G + 1 groups side by side; this kernel has no such pair of
// lanes by construction, and the tests put pieces of G and G + 1 rounds into one wavefront and into neighbouring ones).
//
// Nothing is converted on the way in (as csrc/lsss29.hip.hpp): an operand is its 32 bytes cut into nine limbs (fr_load_raw: below
// 2^256 < 5.3 r, limbs 0..7 in [0, 2^29), limb 8 below 2^24).  In units of r, with r / 2^261 < 0.0059:
//   a round with b    t = (a_i b_i + a_j b_j) / 2^261 (fr_mul2_inline): in (-0.34 r, 1.34 r), limbs 0..7 in [0, 2^29)
//   a round without   t = a_i + a_j, carry-free: below 10.6 r, limbs below 2^30
//   accumulator       acc += t, normalised (fr_norm) after every FR_DOT_NORM = 2 rounds with b and after EVERY round without (a limb stays
//                     below 2^29 + 4 + 2 x 2^29 < 2^31), and reduced by one product with 2^261 mod r (fr_reduce: into (-0.26 r, 1.26 r))
//                     after every FR_DOT_RUN_MUL = 32 rounds with b resp. FR_DOT_RUN_SUM = 4 rounds without: the value stays below
//                     1.26 r + 32 x 1.34 r < 45 r resp. 1.26 r + 4 x 10.6 r < 44 r, its top limb below 45 r / 2^232 < 2^28
//   lane result       with b: acc x 2^522 / 2^261 (fr_to_internal) takes the factor 2^-261 of the products back and reduces in one;
//                     without: fr_reduce.  Columns below 9 x (2^29 + 4) x 2^29 < 2^62; the result is in (-0.27 r, 1.27 r)
//   fold              log2(L) <= six steps v = norm(v + v of lane ^ L/2, .., 1): at most 64 lane results, in (-18 r, 82 r), top limb below 2^28
//   output            fr_reduce: eps = 82 x 0.0059 < 0.49, in (-0.49 r, 1.49 r); fr_canonical<1, 2> takes [-r, 2 r).  Only this is canonical.
// The longest run a lane takes between two reductions is FR_DOT_RUN_MUL rounds whatever the piece's length, which is why the bound does not
// depend on n.  All of it is asserted under -DGPBC_BOUNDS for the interval classes, not for the values of a run.
#ifndef GPBC_FRDOT29_HIP_HPP
#define GPBC_FRDOT29_HIP_HPP
#include "fr29.hip.hpp"
#include "segred29.hip.hpp"

namespace gpbc {

constexpr int FR_DOT_WAVE = 64;                       // lanes of a wavefront, and the most a piece takes
constexpr int FR_DOT_LANES_MIN = 8;                   // ... and the fewest: 8 x 32 bytes are two whole 128-byte lines per load
constexpr int FR_DOT_NORM = 2, FR_DOT_RUN_MUL = 32, FR_DOT_RUN_SUM = 4;
constexpr int FR_DOT_WAVES_PER_SIMD = 4;              // __launch_bounds__ of the kernel: 128 VGPRs
// A piece has at least 512 elements on average, eight per lane (four rounds): below that the two closing products, the fold and the
// canonical store of a piece outweigh its rounds, and 2^20 elements in one segment are still 2048 wavefronts, two per SIMD, with two
// 2 KiB loads per operand each in flight.  `fill` only caps the pieces of one launch and of a very long segment (2^25 elements and
// more): 16 rounds of the 256 CUs x 4 SIMDs x FR_DOT_WAVES_PER_SIMD wavefronts that are resident at once, so that 2^16 short segments
// are one launch and not sixteen.  There are no tables: a piece costs 32 bytes of workspace.
constexpr SegRedShape FR_DOT_SHAPE{16 * 256 * 4 * FR_DOT_WAVES_PER_SIMD, 512, 512};

// the 32 bytes of element i: `wide` = the base address is 16-byte aligned
GPBC_INLINE Fr fr_dot_load(const uint8_t *base, size_t i, bool wide) {
    const uint8_t *p = base + 32 * i;
#if defined(__HIP_DEVICE_COMPILE__)
    if (wide) {
        const uint4 lo = reinterpret_cast<const uint4 *>(p)[0], hi = reinterpret_cast<const uint4 *>(p)[1];
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        return fr_load_raw(reinterpret_cast<const uint8_t *>(w));
    }
#else
    (void)wide;
#endif
    return fr_load_raw(p);
}

// The partial sum of lane `lane` over the piece [a, b) of x (and of k, whose element for x[i] is k[i - k0]; k null: plain sum).
// L lanes share the piece, `lane` is this one's place among them; `rounds` is the wavefront's trip count, the largest
// fr_dot_rounds(b - a, L) of its pieces.  The result is reduced: in (-0.27 r, 1.27 r), not canonical.
GPBC_INLINE size_t fr_dot_rounds(size_t len, uint32_t L) { return (len + 2 * L - 1) / (2 * L); }
// lanes per piece of one launch, from the sizes alone: the mean piece has at most two elements per lane where that is possible
GPBC_INLINE uint32_t fr_dot_lanes(const SegRedArgs &g) {
    const size_t per_segment = g.seg_off ? (g.n_seg ? g.n / g.n_seg : 0) : g.m, mean = per_segment / (g.J ? g.J : 1);
    uint32_t L = FR_DOT_LANES_MIN;
    while (L < (uint32_t)FR_DOT_WAVE && 2 * (size_t)L < mean) L <<= 1;
    return L;
}
GPBC_INLINE Fr fr_dot_lane(const uint8_t *x, const uint8_t *k, size_t k0, size_t a, size_t b, uint32_t lane, uint32_t L, size_t rounds, bool wide_x, bool wide_k) {
    Fr acc = fr_zero();
    int pending = 0, run = 0;
    const int run_max = k ? FR_DOT_RUN_MUL : FR_DOT_RUN_SUM, norm_max = k ? FR_DOT_NORM : 1;
    size_t i = a + lane;
    for (size_t t = 0; t < rounds; t++, i += 2 * (size_t)L) {
        const size_t j = i + L;
        // an element past the end is zero: its lane runs the round like every other
        Fr xi = fr_zero(), xj = xi;
        if (i < b) xi = fr_dot_load(x, i, wide_x);
        if (j < b) xj = fr_dot_load(x, j, wide_x);
        if (k) {
            Fr ki = fr_zero(), kj = ki;
            if (i < b) ki = fr_dot_load(k, i - k0, wide_k);
            if (j < b) kj = fr_dot_load(k, j - k0, wide_k);
            acc = fr_add(acc, fr_mul2_inline(xi, ki, xj, kj));
        } else {
            acc = fr_add(acc, fr_add(xi, xj));
        }
        if (++pending == norm_max) { acc = fr_norm(acc); pending = 0; }
        if (++run == run_max) { acc = fr_reduce(fr_norm(acc)); pending = 0; run = 0; }
    }
    acc = fr_norm(acc);
    return k ? fr_to_internal(acc) : fr_reduce(acc);
}
// one step of the fold, and the way out
GPBC_INLINE Fr fr_dot_fold(const Fr &v, const Fr &other) { return fr_norm(fr_add(v, other)); }
GPBC_INLINE void fr_dot_store(uint8_t *out, const Fr &folded) { fr_store_canonical(out, fr_canonical<1, 2>(fr_reduce(folded))); }

}  // namespace gpbc
#endif
