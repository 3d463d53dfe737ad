// libgpbc_bn254.so, one of the units listed in _build.py: gnark wire formats (csrc/wire29.hip.hpp) and hash to curve — hash_to_field
// (csrc/xmd29.hip.hpp) and the group part (csrc/h2c29.hip.hpp) — with their C-ABI entries (include/gpbc_bn254.h); and, as the unit
// that has the GT coefficient order and fe_to_plain_words, the XOR mask from GT bytes (csrc/mask29.hip.hpp) with the entries of
// include/gpbc_bn254_mask.h.  gfx950 only.
#include "gpbc_common.hpp"
#include "../../include/gpbc_bn254_mask.h"
#include "curve29_oct.hip.hpp"
#include "wire29.hip.hpp"
#include "h2c29.hip.hpp"
#include "xmd29.hip.hpp"
#include "mask29.hip.hpp"

// ---- wire formats (csrc/wire29.hip.hpp): one element per lane
GPBC_KERNEL k_g1_encode(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, size_t n, int compressed) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    g1_wire_encode(out + i * (compressed ? GPBC_G1_COMPRESSED_BYTES : GPBC_G1_RAW_BYTES), in + i * GPBC_G1_BYTES, compressed != 0);
}
GPBC_KERNEL k_g2_encode(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, size_t n, int compressed) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    g2_wire_encode(out + i * (compressed ? GPBC_G2_COMPRESSED_BYTES : GPBC_G2_RAW_BYTES), in + i * GPBC_G2_BYTES, compressed != 0);
}
GPBC_KERNEL k_gt_encode(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    gt_wire_encode(out + i * GPBC_GT_BYTES, in + i * GPBC_GT_BYTES);
}
GPBC_KERNEL k_g1_decode(const uint8_t *__restrict__ in, int elem_bytes, uint8_t *__restrict__ out, uint8_t *__restrict__ ok, size_t n) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    ok[i] = g1_wire_decode(out + i * GPBC_G1_BYTES, in + i * (size_t)elem_bytes, elem_bytes) ? 1 : 0;
}
GPBC_KERNEL k_g2_decode(const uint8_t *__restrict__ in, int elem_bytes, uint8_t *__restrict__ out, uint8_t *__restrict__ ok, size_t n) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    ok[i] = g2_wire_decode(out + i * GPBC_G2_BYTES, in + i * (size_t)elem_bytes, elem_bytes) ? 1 : 0;
}
// G2 decoding with one element per QUAD of lanes (calls of up to WIRE_QUAD_MAX elements): the 63-bit double-and-add of the subgroup
// test — two thirds of a decode — three products wide (csrc/curve29_quad.hip.hpp); the four lanes decode the same element and take
// the same branches.
constexpr size_t WIRE_QUAD_MAX = 16384;
__device__ __forceinline__ bool g2_in_subgroup29_quad(const F2 &x, const F2 &y, int q) {
    constexpr uint64_t X = 4965661367192848881ull;
    AffP<F2> pt{x, y, false};
    JacP<F2> xq;
    jac_set_inf(xq);
    for (int i = 62; i >= 0; i--) {
        jac_dbl_quad(xq, q);
        if ((X >> i) & 1) jac_add_mixed_quad(xq, pt, q);
    }
    JacP<F2> lhs, t, rhs;
    jac_add_mixed(lhs, xq, pt);                                  // [x+1]Q
    jac_add(lhs, lhs, jac_psi_tw(xq, 1));
    jac_add(lhs, lhs, jac_psi_tw(xq, 2));
    jac_dbl(t, xq);
    rhs = jac_psi_tw(t, 3);
    if (!rhs.inf) rhs.y = f2_neg(rhs.y);
    jac_add(t, lhs, rhs);                                        // lhs - rhs
    return t.inf;
}
GPBC_KERNEL k_g2_decode_quad(const uint8_t *__restrict__ in, int elem_bytes, uint8_t *__restrict__ out, uint8_t *__restrict__ ok, size_t n) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x, i = lane >> 2;
    if (i >= n) return;
    const int q = (int)(lane & 3);
    const bool good = g2_wire_decode(out + i * GPBC_G2_BYTES, in + i * (size_t)elem_bytes, elem_bytes, [&](const F2 &x, const F2 &y) { return g2_in_subgroup29_quad(x, y, q); });
    if (q == 0) ok[i] = good ? 1 : 0;                            // (the four lanes wrote the same point bytes)
}
// ... and with one element per OCTET (calls of up to WIRE_OCT_MAX elements: one Unmarshal): the same chain with the two halves of every
// Fp2 product on two lanes (csrc/curve29_oct.hip.hpp)
constexpr size_t WIRE_OCT_MAX = 2048;
__device__ __forceinline__ bool g2_in_subgroup29_oct(const F2 &x, const F2 &y, int q) {
    constexpr uint64_t X = 4965661367192848881ull;
    AffP<F2> pt{x, y, false};
    JacP<F2> xq;
    jac_set_inf(xq);
    for (int i = 62; i >= 0; i--) {
        jac_dbl_oct(xq, q);
        if ((X >> i) & 1) jac_add_mixed_oct(xq, pt, q);
    }
    JacP<F2> lhs = xq, t, rhs;
    jac_add_mixed_oct(lhs, pt, q);                               // [x+1]Q
    jac_add(lhs, lhs, jac_psi_tw(xq, 1));
    jac_add(lhs, lhs, jac_psi_tw(xq, 2));
    t = xq;
    jac_dbl_oct(t, q);
    rhs = jac_psi_tw(t, 3);
    if (!rhs.inf) rhs.y = f2_neg(rhs.y);
    jac_add(t, lhs, rhs);                                        // lhs - rhs
    return t.inf;
}
GPBC_KERNEL k_g2_decode_oct(const uint8_t *__restrict__ in, int elem_bytes, uint8_t *__restrict__ out, uint8_t *__restrict__ ok, size_t n) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x, i = lane >> 3;
    if (i >= n) return;
    const int q = (int)(lane & 7);
    const bool good = g2_wire_decode(out + i * GPBC_G2_BYTES, in + i * (size_t)elem_bytes, elem_bytes, [&](const F2 &x, const F2 &y) { return g2_in_subgroup29_oct(x, y, q); });
    if (q == 0) ok[i] = good ? 1 : 0;
}
GPBC_KERNEL k_gt_decode(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, uint8_t *__restrict__ ok, size_t n) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    ok[i] = gt_wire_decode(out + i * GPBC_GT_BYTES, in + i * GPBC_GT_BYTES) ? 1 : 0;
}

// ---- hash to curve, group part (csrc/h2c29.hip.hpp): u = n x 2 field elements -> n points
GPBC_KERNEL k_g1_map_fields(const uint8_t *__restrict__ u, uint8_t *__restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    AffP<Fe> r;
    g1_map_fields(r, fe_load(u + i * 64), fe_load(u + i * 64 + 32));
    g1_store_aff(out + i * GPBC_G1_BYTES, r);
}
GPBC_KERNEL k_g2_map_fields(const uint8_t *__restrict__ u, uint8_t *__restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    AffP<F2> r;
    g2_map_fields(r, f2_load(u + i * 128), f2_load(u + i * 128 + 64));
    g2_store_aff(out + i * GPBC_G2_BYTES, r);
}

// ---- hash to curve, whole (csrc/xmd29.hip.hpp + h2c29.hip.hpp): one message per lane.  Message i is msgs[off[i], off[i+1]),
// clamped to the buffer by msg_range (xmd29.hip.hpp).
template <int COUNT> GPBC_KERNEL k_hash_to_field(const uint8_t *__restrict__ msgs, const uint64_t *__restrict__ off, size_t total, size_t n, XmdDst dst,
                                                 uint8_t *__restrict__ out) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint64_t lo, len;
    msg_range(off, total, i, lo, len);
    uint32_t u[COUNT * 12];
    expand_message_xmd<COUNT * 12 / 8>(u, msgs + lo, len, dst);
#pragma unroll
    for (int e = 0; e < COUNT; e++) fe_store(out + (i * COUNT + e) * 32, xmd_field(u, e));
}
GPBC_KERNEL k_g1_hash(const uint8_t *__restrict__ msgs, const uint64_t *__restrict__ off, size_t total, size_t n, XmdDst dst, uint8_t *__restrict__ out) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint64_t lo, len;
    msg_range(off, total, i, lo, len);
    uint32_t u[24];
    expand_message_xmd<3>(u, msgs + lo, len, dst);
    AffP<Fe> r;
    g1_map_fields(r, xmd_field(u, 0), xmd_field(u, 1));
    g1_store_aff(out + i * GPBC_G1_BYTES, r);
}
GPBC_KERNEL k_g2_hash(const uint8_t *__restrict__ msgs, const uint64_t *__restrict__ off, size_t total, size_t n, XmdDst dst, uint8_t *__restrict__ out) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint64_t lo, len;
    msg_range(off, total, i, lo, len);
    uint32_t u[48];
    expand_message_xmd<6>(u, msgs + lo, len, dst);
    AffP<F2> r;
    g2_map_fields(r, F2{xmd_field(u, 0), xmd_field(u, 1)}, F2{xmd_field(u, 2), xmd_field(u, 3)});
    g2_store_aff(out + i * GPBC_G2_BYTES, r);
}

// ---- the same with one message (or one pair of field elements) per QUAD of lanes, for calls of up to H2C_QUAD_MAX: lanes 0 and 1 map
// u0 and u1 side by side (each map is a chain of ~300 (G1) / ~650 (G2) dependent Fp products, most of it the square root), and the
// 63 doublings and 30 additions of G2's cofactor clearing run three products wide (csrc/curve29_quad.hip.hpp).  One call of
// HashToG1 / HashToG2 — what bls01's Sign and Verify make — 0.9 / 2.8 -> 0.6 / 1.4 ms.
constexpr size_t H2C_QUAD_MAX = 16384;
template <class F> __device__ __forceinline__ void map_pair_quad(AffP<F> &q0, AffP<F> &q1, const F &u0, const F &u1, int q) {
    AffP<F> m;
    map_to_curve_svdw<F>(m, g_sel<F>((q & 1) != 0, u1, u0));
    q0 = AffP<F>{quad_bcast<0>(m.x), quad_bcast<0>(m.y), false};
    q1 = AffP<F>{quad_bcast<1>(m.x), quad_bcast<1>(m.y), false};
}
__device__ __forceinline__ void g1_map_fields_quad(AffP<Fe> &out, const Fe &u0, const Fe &u1, int q) {
    AffP<Fe> q0, q1;
    map_pair_quad<Fe>(q0, q1, u0, u1, q);
    JacP<Fe> j{q0.x, q0.y, fe_one(), false}, s;
    jac_add_mixed(s, j, q1);
    jac_to_affine(out, s);
}
// g2_clear_cofactor29 with the [x]P chain on the quad
__device__ __forceinline__ void g2_clear_cofactor29_quad(JacP<F2> &out, const AffP<F2> &p, int q) {
    constexpr uint64_t X = 4965661367192848881ull;
    JacP<F2> xq, t;
    jac_set_inf(xq);
    for (int i = 62; i >= 0; i--) {
        jac_dbl_quad(xq, q);
        if ((X >> i) & 1) jac_add_mixed_quad(xq, p, q);
    }
    jac_dbl(t, xq);
    jac_add(t, t, xq);                                          // [3x]P
    JacP<F2> pj{p.x, p.y, f2_one(), p.inf};
    JacP<F2> acc;
    jac_add(acc, xq, jac_psi(t, 1));
    jac_add(acc, acc, jac_psi(xq, 2));
    jac_add(out, acc, jac_psi(pj, 3));
}
__device__ __forceinline__ void g2_map_fields_quad(AffP<F2> &out, const F2 &u0, const F2 &u1, int q) {
    AffP<F2> q0, q1, a;
    map_pair_quad<F2>(q0, q1, u0, u1, q);
    JacP<F2> j{q0.x, q0.y, f2_one(), false}, s, c;
    jac_add_mixed(s, j, q1);
    jac_to_affine(a, s);
    g2_clear_cofactor29_quad(c, a, q);
    jac_to_affine(out, c);
}
// ... and G2 with one message per OCTET (calls of up to H2C_OCT_MAX messages: the HashToG2 of one Sign or Verify): lanes q & 1 map u0 / u1,
// the [x]P chain of the cofactor clearing runs on half products (csrc/curve29_oct.hip.hpp)
constexpr size_t H2C_OCT_MAX = 2048;
__device__ __forceinline__ void g2_clear_cofactor29_oct(JacP<F2> &out, const AffP<F2> &p, int q) {
    constexpr uint64_t X = 4965661367192848881ull;
    JacP<F2> xq, t;
    jac_set_inf(xq);
    for (int i = 62; i >= 0; i--) {
        jac_dbl_oct(xq, q);
        if ((X >> i) & 1) jac_add_mixed_oct(xq, p, q);
    }
    t = xq;
    jac_dbl_oct(t, q);
    jac_add(t, t, xq);                                          // [3x]P
    JacP<F2> pj{p.x, p.y, f2_one(), p.inf};
    JacP<F2> acc;
    jac_add(acc, xq, jac_psi(t, 1));
    jac_add(acc, acc, jac_psi(xq, 2));
    jac_add(out, acc, jac_psi(pj, 3));
}
__device__ __forceinline__ void g2_map_fields_oct(AffP<F2> &out, const F2 &u0, const F2 &u1, int q) {
    AffP<F2> q0, q1, a;
    map_pair_quad<F2>(q0, q1, u0, u1, q & 3);                   // (each quad of the octet maps both: lanes 0 / 1 and 4 / 5)
    JacP<F2> s{q0.x, q0.y, f2_one(), false}, c;
    jac_add_mixed_oct(s, q1, q);
    jac_to_affine(a, s);
    g2_clear_cofactor29_oct(c, a, q);
    jac_to_affine(out, c);
}
GPBC_KERNEL k_g2_map_fields_oct(const uint8_t *__restrict__ u, uint8_t *__restrict__ out, size_t n) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x, i = lane >> 3;
    if (i >= n) return;
    AffP<F2> r;
    g2_map_fields_oct(r, f2_load(u + i * 128), f2_load(u + i * 128 + 64), (int)(lane & 7));
    if ((lane & 7) == 0) g2_store_aff(out + i * GPBC_G2_BYTES, r);
}
GPBC_KERNEL k_g2_hash_oct(const uint8_t *__restrict__ msgs, const uint64_t *__restrict__ off, size_t total, size_t n, XmdDst dst, uint8_t *__restrict__ out) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x, i = lane >> 3;
    if (i >= n) return;
    uint64_t lo, len;
    msg_range(off, total, i, lo, len);
    uint32_t u[48];
    expand_message_xmd<6>(u, msgs + lo, len, dst);
    AffP<F2> r;
    g2_map_fields_oct(r, F2{xmd_field(u, 0), xmd_field(u, 1)}, F2{xmd_field(u, 2), xmd_field(u, 3)}, (int)(lane & 7));
    if ((lane & 7) == 0) g2_store_aff(out + i * GPBC_G2_BYTES, r);
}
GPBC_KERNEL k_g1_map_fields_quad(const uint8_t *__restrict__ u, uint8_t *__restrict__ out, size_t n) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x, i = lane >> 2;
    if (i >= n) return;
    AffP<Fe> r;
    g1_map_fields_quad(r, fe_load(u + i * 64), fe_load(u + i * 64 + 32), (int)(lane & 3));
    if ((lane & 3) == 0) g1_store_aff(out + i * GPBC_G1_BYTES, r);
}
GPBC_KERNEL k_g2_map_fields_quad(const uint8_t *__restrict__ u, uint8_t *__restrict__ out, size_t n) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x, i = lane >> 2;
    if (i >= n) return;
    AffP<F2> r;
    g2_map_fields_quad(r, f2_load(u + i * 128), f2_load(u + i * 128 + 64), (int)(lane & 3));
    if ((lane & 3) == 0) g2_store_aff(out + i * GPBC_G2_BYTES, r);
}
GPBC_KERNEL k_g1_hash_quad(const uint8_t *__restrict__ msgs, const uint64_t *__restrict__ off, size_t total, size_t n, XmdDst dst, uint8_t *__restrict__ out) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x, i = lane >> 2;
    if (i >= n) return;
    uint64_t lo, len;
    msg_range(off, total, i, lo, len);
    uint32_t u[24];
    expand_message_xmd<3>(u, msgs + lo, len, dst);
    AffP<Fe> r;
    g1_map_fields_quad(r, xmd_field(u, 0), xmd_field(u, 1), (int)(lane & 3));
    if ((lane & 3) == 0) g1_store_aff(out + i * GPBC_G1_BYTES, r);
}
GPBC_KERNEL k_g2_hash_quad(const uint8_t *__restrict__ msgs, const uint64_t *__restrict__ off, size_t total, size_t n, XmdDst dst, uint8_t *__restrict__ out) {
    const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x, i = lane >> 2;
    if (i >= n) return;
    uint64_t lo, len;
    msg_range(off, total, i, lo, len);
    uint32_t u[48];
    expand_message_xmd<6>(u, msgs + lo, len, dst);
    AffP<F2> r;
    g2_map_fields_quad(r, F2{xmd_field(u, 0), xmd_field(u, 1)}, F2{xmd_field(u, 2), xmd_field(u, 3)}, (int)(lane & 3));
    if ((lane & 3) == 0) g2_store_aff(out + i * GPBC_G2_BYTES, r);
}

// ---- the XOR mask from GT bytes (csrc/mask29.hip.hpp): one lane per (item, 32-byte window).  Rows: wpi lanes per item, an item's lanes
// side by side.  Offsets: twelve lanes per item, a WAVEFRONT per window of 64 items (mask_ragged_lane), so that the wavefronts of
// windows no message of the 64 reaches leave after two loads.
__global__ void __launch_bounds__(MASK_BLOCK) k_gt_xor_mask(const uint8_t *__restrict__ gt, const uint8_t *msgs, const uint64_t *off, size_t total, size_t width, size_t n,
                                                            int wpi, uint8_t *out, uint32_t *out_len) {
    const size_t lane = (size_t)blockIdx.x * MASK_BLOCK + threadIdx.x;
    size_t i;
    int w;
    if (off) mask_ragged_lane(lane, i, w);
    else { i = lane / (unsigned)wpi; w = (int)(lane - i * (unsigned)wpi); }
    if (i >= n) return;
    gt_xor_mask_lane(gt, msgs, off, total, width, i, w, out, out_len);
}

extern "C" {

// ----------------------------------------------------------------------------------------------- wire formats
// kind 0 = G1, 1 = G2, 2 = GT
static size_t wire_mem_bytes(int kind) { return kind == 0 ? GPBC_G1_BYTES : kind == 1 ? GPBC_G2_BYTES : GPBC_GT_BYTES; }
static size_t wire_enc_bytes(int kind, int compressed) {
    return kind == 0 ? (compressed ? GPBC_G1_COMPRESSED_BYTES : GPBC_G1_RAW_BYTES)
         : kind == 1 ? (compressed ? GPBC_G2_COMPRESSED_BYTES : GPBC_G2_RAW_BYTES) : GPBC_GT_BYTES;
}
static int marshal_dev(int kind, const void *d_in, size_t n, int compressed, void *d_out, void *stream) {
    if (!n) return GPBC_OK;
    if (!d_in || !d_out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    if (d_in == d_out) return fail(GPBC_ERR_INVALID_ARG, "marshal cannot run in place");
    TRY(bind_device());
    hipStream_t st = (hipStream_t)stream;
    if (kind == 0) return GPBC_LAUNCH(k_g1_encode, grid_for(n), BLOCK, st, (const uint8_t *)d_in, (uint8_t *)d_out, n, compressed);
    if (kind == 1) return GPBC_LAUNCH(k_g2_encode, grid_for(n), BLOCK, st, (const uint8_t *)d_in, (uint8_t *)d_out, n, compressed);
    return GPBC_LAUNCH(k_gt_encode, grid_for(n), BLOCK, st, (const uint8_t *)d_in, (uint8_t *)d_out, n);
}
static int unmarshal_dev(int kind, const void *d_in, size_t elem_bytes, size_t n, void *d_out, uint8_t *d_ok, void *stream) {
    if (kind == 0 && elem_bytes != GPBC_G1_COMPRESSED_BYTES && elem_bytes != GPBC_G1_RAW_BYTES)
        return fail(GPBC_ERR_INVALID_ARG, "G1 element size must be 32 or 64");
    if (kind == 1 && elem_bytes != GPBC_G2_COMPRESSED_BYTES && elem_bytes != GPBC_G2_RAW_BYTES)
        return fail(GPBC_ERR_INVALID_ARG, "G2 element size must be 64 or 128");
    if (!n) return GPBC_OK;
    if (!d_in || !d_out || !d_ok) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    if (d_in == d_out) return fail(GPBC_ERR_INVALID_ARG, "unmarshal cannot run in place");
    TRY(bind_device());
    hipStream_t st = (hipStream_t)stream;
    const uint8_t *in = (const uint8_t *)d_in;
    if (kind == 0) return GPBC_LAUNCH(k_g1_decode, grid_for(n), BLOCK, st, in, (int)elem_bytes, (uint8_t *)d_out, d_ok, n);
    if (kind == 1 && n <= WIRE_OCT_MAX) return GPBC_LAUNCH(k_g2_decode_oct, grid_for(8 * n), BLOCK, st, in, (int)elem_bytes, (uint8_t *)d_out, d_ok, n);
    if (kind == 1 && n <= WIRE_QUAD_MAX) return GPBC_LAUNCH(k_g2_decode_quad, grid_for(4 * n), BLOCK, st, in, (int)elem_bytes, (uint8_t *)d_out, d_ok, n);
    if (kind == 1) return GPBC_LAUNCH(k_g2_decode, grid_for(n), BLOCK, st, in, (int)elem_bytes, (uint8_t *)d_out, d_ok, n);
    return GPBC_LAUNCH(k_gt_decode, grid_for(n), BLOCK, st, in, (uint8_t *)d_out, d_ok, n);
}
// host-pointer entries shard [0, n) over the bound devices (run_sharded, gpbc_core.hip); a small call goes through a call lane (pinned
// block in and out, the lane's stream), gpbc_common.hpp
constexpr size_t WIRE_SHARD_MIN = 65536;
static int marshal_host(int kind, const void *in, size_t n, int compressed, void *out) {
    if (!n) return GPBC_OK;
    if (!in || !out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    return host_call_sharded(n, WIRE_SHARD_MIN, HostCall().input(in, wire_mem_bytes(kind)).output(out, wire_enc_bytes(kind, compressed)),
                             HostRoute{CALL_KINDS, nullptr, 0, LANE_CALL_MAX_UNITS},
                             [=](const DevCols &d, size_t m, hipStream_t st) { return marshal_dev(kind, d.in[0], m, compressed, d.out[0], st); });
}
static int unmarshal_host(int kind, const void *in, size_t elem_bytes, size_t n, void *out, uint8_t *ok) {
    if (!n) return unmarshal_dev(kind, nullptr, elem_bytes, 0, nullptr, nullptr, nullptr);      // (still rejects a bad elem_bytes)
    if (!in || !out || !ok) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    const size_t min_units = kind == 1 ? 8192 : WIRE_SHARD_MIN;                 // G2 decoding carries the subgroup check
    return host_call_sharded(n, min_units, HostCall().input(in, elem_bytes).output(out, wire_mem_bytes(kind)).output(ok, 1),
                             HostRoute{CALL_KINDS, nullptr, 0, LANE_CALL_MAX_UNITS},
                             [=](const DevCols &d, size_t m, hipStream_t st) { return unmarshal_dev(kind, d.in[0], elem_bytes, m, d.out[0], d.out[1], st); });
}
int gpbc_g1_marshal_batch(const void *p, size_t n, int c, void *o) { return marshal_host(0, p, n, c != 0, o); }
int gpbc_g2_marshal_batch(const void *p, size_t n, int c, void *o) { return marshal_host(1, p, n, c != 0, o); }
int gpbc_gt_marshal_batch(const void *g, size_t n, void *o) { return marshal_host(2, g, n, 0, o); }
int gpbc_g1_marshal_batch_dev(const void *p, size_t n, int c, void *o, void *st) { return marshal_dev(0, p, n, c != 0, o, st); }
int gpbc_g2_marshal_batch_dev(const void *p, size_t n, int c, void *o, void *st) { return marshal_dev(1, p, n, c != 0, o, st); }
int gpbc_gt_marshal_batch_dev(const void *g, size_t n, void *o, void *st) { return marshal_dev(2, g, n, 0, o, st); }
int gpbc_g1_unmarshal_batch(const void *in, size_t eb, size_t n, void *o, uint8_t *ok) { return unmarshal_host(0, in, eb, n, o, ok); }
int gpbc_g2_unmarshal_batch(const void *in, size_t eb, size_t n, void *o, uint8_t *ok) { return unmarshal_host(1, in, eb, n, o, ok); }
int gpbc_gt_unmarshal_batch(const void *in, size_t n, void *o, uint8_t *ok) { return unmarshal_host(2, in, GPBC_GT_BYTES, n, o, ok); }
int gpbc_g1_unmarshal_batch_dev(const void *in, size_t eb, size_t n, void *o, uint8_t *ok, void *st) { return unmarshal_dev(0, in, eb, n, o, ok, st); }
int gpbc_g2_unmarshal_batch_dev(const void *in, size_t eb, size_t n, void *o, uint8_t *ok, void *st) { return unmarshal_dev(1, in, eb, n, o, ok, st); }
int gpbc_gt_unmarshal_batch_dev(const void *in, size_t n, void *o, uint8_t *ok, void *st) { return unmarshal_dev(2, in, GPBC_GT_BYTES, n, o, ok, st); }

// ----------------------------------------------------------------------------------------------- hash to curve (group part)
static int map_fields_dev(bool g2, const void *d_u, size_t n, void *d_out, void *stream) {
    if (!n) return GPBC_OK;
    if (!d_u || !d_out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    TRY(bind_device());
    const hipStream_t st = (hipStream_t)stream;
    const uint8_t *u = (const uint8_t *)d_u;
    if (g2 && n <= H2C_OCT_MAX) return GPBC_LAUNCH(k_g2_map_fields_oct, grid_for(8 * n), BLOCK, st, u, (uint8_t *)d_out, n);
    if (g2 && n <= H2C_QUAD_MAX) return GPBC_LAUNCH(k_g2_map_fields_quad, grid_for(4 * n), BLOCK, st, u, (uint8_t *)d_out, n);
    if (n <= H2C_QUAD_MAX) return GPBC_LAUNCH(k_g1_map_fields_quad, grid_for(4 * n), BLOCK, st, u, (uint8_t *)d_out, n);
    if (g2) return GPBC_LAUNCH(k_g2_map_fields, grid_for(n), BLOCK, st, u, (uint8_t *)d_out, n);
    return GPBC_LAUNCH(k_g1_map_fields, grid_for(n), BLOCK, st, u, (uint8_t *)d_out, n);
}
static int map_fields_host(bool g2, const void *u, size_t n, void *out) {
    if (!n) return GPBC_OK;
    if (!u || !out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    const size_t pt = g2 ? GPBC_G2_BYTES : GPBC_G1_BYTES;               // two field elements occupy as many bytes as one point
    return host_call_sharded(n, 8192, HostCall().input(u, pt).output(out, pt), HostRoute{CALL_KINDS, nullptr, 0, LANE_CALL_MAX_UNITS},
                             [=](const DevCols &d, size_t m, hipStream_t st) { return map_fields_dev(g2, d.in[0], m, d.out[0], st); });
}
int gpbc_g1_map_to_curve_batch(const void *u, size_t n, void *o) { return map_fields_host(false, u, n, o); }
int gpbc_g2_map_to_curve_batch(const void *u, size_t n, void *o) { return map_fields_host(true, u, n, o); }
int gpbc_g1_map_to_curve_batch_dev(const void *u, size_t n, void *o, void *st) { return map_fields_dev(false, u, n, o, st); }
int gpbc_g2_map_to_curve_batch_dev(const void *u, size_t n, void *o, void *st) { return map_fields_dev(true, u, n, o, st); }

// ----------------------------------------------------------------------------------------------- hash to curve (whole) and hash to field
// what: 0 = G1 points, 1 = G2 points, 2 / 4 = that many field elements per message
static size_t hash_out_bytes(int what) { return what == 0 ? GPBC_G1_BYTES : what == 1 ? GPBC_G2_BYTES : (size_t)what * 32; }
static int hash_dev(int what, const void *d_msgs, const uint64_t *d_off, size_t msgs_bytes, size_t n, const void *dst, size_t dst_len, void *d_out, void *stream) {
    if (!n) return GPBC_OK;
    if (!d_off || !d_out || (msgs_bytes && !d_msgs) || (dst_len && !dst)) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    if (dst_len > 255) return fail(GPBC_ERR_INVALID_ARG, "DST longer than 255 bytes: hash it down first (RFC 9380 section 5.3.3)");
    TRY(bind_device());
    XmdDst d;
    memset(&d, 0, sizeof d);
    if (dst_len) memcpy(d.b, dst, dst_len);                      // dst == NULL with dst_len == 0 is a legal (empty) tag
    d.len = (uint32_t)dst_len;
    hipStream_t st = (hipStream_t)stream;
    const uint8_t *m = (const uint8_t *)d_msgs;
    uint8_t *o = (uint8_t *)d_out;
    switch (what) {
        case 0: if (n <= H2C_QUAD_MAX) return GPBC_LAUNCH(k_g1_hash_quad, grid_for(4 * n), BLOCK, st, m, d_off, msgs_bytes, n, d, o);
                return GPBC_LAUNCH(k_g1_hash, grid_for(n), BLOCK, st, m, d_off, msgs_bytes, n, d, o);
        case 1: if (n <= H2C_OCT_MAX) return GPBC_LAUNCH(k_g2_hash_oct, grid_for(8 * n), BLOCK, st, m, d_off, msgs_bytes, n, d, o);
                if (n <= H2C_QUAD_MAX) return GPBC_LAUNCH(k_g2_hash_quad, grid_for(4 * n), BLOCK, st, m, d_off, msgs_bytes, n, d, o);
                return GPBC_LAUNCH(k_g2_hash, grid_for(n), BLOCK, st, m, d_off, msgs_bytes, n, d, o);
        case 2: return GPBC_LAUNCH(k_hash_to_field<2>, grid_for(n), BLOCK, st, m, d_off, msgs_bytes, n, d, o);
        case 4: return GPBC_LAUNCH(k_hash_to_field<4>, grid_for(n), BLOCK, st, m, d_off, msgs_bytes, n, d, o);
        default: return fail(GPBC_ERR_INVALID_ARG, "count must be 2 or 4");
    }
}
// Small calls of HashToG1 / HashToG2 (every BLS Sign and Verify starts with one: signature/bls01_signature/bls_signature.go:58-63,75-79) are
// COMBINED like the pairings (gpbc_common.hpp "Small host-pointer calls"): requests with the same domain-separation tag — the key —
// share one launch; in[0] = the call's message bytes, seg = its offsets (rebased to 0), units = messages.
static int small_hash_run(SmallKind kind, CallLane &lane, SmallCall *const *calls, size_t nc) {
    const int what = kind == CALL_HASH_G2 ? 1 : 0;
    size_t N = 0, B = 0;
    for (size_t c = 0; c < nc; c++) { N += calls[c]->units; B += (size_t)calls[c]->seg[calls[c]->units]; }
    const size_t ob = hash_out_bytes(what), o_off = Scratch::padded(B), o_out = o_off + Scratch::padded((N + 1) * sizeof(uint64_t));
    TRY(lane.reserve(o_out + Scratch::padded(N * ob), 0));
    uint64_t *off = (uint64_t *)(lane.pin + o_off);
    size_t n0 = 0, b0 = 0;
    for (size_t c = 0; c < nc; c++) {
        const SmallCall &r = *calls[c];
        const size_t bytes = (size_t)r.seg[r.units];
        if (bytes) memcpy(lane.pin + b0, r.in[0], bytes);
        for (size_t i = 0; i < r.units; i++) off[n0 + i] = b0 + r.seg[i];
        n0 += r.units; b0 += bytes;
    }
    off[N] = B;
    TRY(hash_dev(what, lane.d_pin, (const uint64_t *)(lane.d_pin + o_off), B, N, calls[0]->key, calls[0]->key_len, lane.d_pin + o_out, lane.stream));
    HIP_TRY(hipStreamSynchronize(lane.stream));
    n0 = 0;
    for (size_t c = 0; c < nc; c++) { memcpy(calls[c]->out[0], lane.pin + o_out + n0 * ob, calls[c]->units * ob); n0 += calls[c]->units; }
    return GPBC_OK;
}
static int hash_host(int what, const void *msgs, const uint64_t *off, size_t n, const void *dst, size_t dst_len, void *out) {
    if (!n) return GPBC_OK;
    if (!off || !out || (dst_len && !dst)) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    for (size_t i = 0; i < n; i++) if (off[i + 1] < off[i]) return fail(GPBC_ERR_INVALID_ARG, "message offsets must not decrease");
    if (off[n] > off[0] && !msgs) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    const size_t ob = hash_out_bytes(what);
    return run_sharded(n, 8192, [=](size_t lo, size_t hi) {
        // a shard's messages and its offsets rebased to them, both whole columns; combined calls up to 1 MiB of messages, a lane up to 64 MiB
        const size_t m = hi - lo;
        const uint64_t base = off[lo], bytes = off[hi] - base;
        std::vector<uint64_t> rel(m + 1);
        for (size_t i = 0; i <= m; i++) rel[i] = off[lo + i] - base;
        HostCall c = HostCall().input((const uint8_t *)msgs + base, bytes, true).input(rel.data(), (m + 1) * sizeof(uint64_t), true).output((uint8_t *)out + lo * ob, ob);
        c.seg = rel.data(); c.key = dst; c.key_len = dst_len;
        const bool combined = (what == 0 || what == 1) && bytes <= ((size_t)1 << 20) && dst_len <= 255;
        const HostRoute r{what == 1 ? CALL_HASH_G2 : CALL_HASH_G1, small_hash_run, combined ? SMALL_CALL_MAX_UNITS : 0, bytes <= ((size_t)64 << 20) ? LANE_CALL_MAX_UNITS : 0};
        return host_call(m, c, r, [&](const DevCols &d, size_t, hipStream_t st) {
            return hash_dev(what, d.in[0], (const uint64_t *)d.in[1], bytes, m, dst, dst_len, d.out[0], st);
        });
    });
}
int gpbc_hash_to_g1(const void *m, const uint64_t *off, size_t n, const void *dst, size_t dl, void *o) { return hash_host(0, m, off, n, dst, dl, o); }
int gpbc_hash_to_g2(const void *m, const uint64_t *off, size_t n, const void *dst, size_t dl, void *o) { return hash_host(1, m, off, n, dst, dl, o); }
int gpbc_hash_to_field(const void *m, const uint64_t *off, size_t n, const void *dst, size_t dl, int count, void *o) {
    if (count != 2 && count != 4) return fail(GPBC_ERR_INVALID_ARG, "count must be 2 or 4");
    return hash_host(count, m, off, n, dst, dl, o);
}
int gpbc_hash_to_g1_dev(const void *m, const uint64_t *off, size_t mb, size_t n, const void *dst, size_t dl, void *o, void *st) { return hash_dev(0, m, off, mb, n, dst, dl, o, st); }
int gpbc_hash_to_g2_dev(const void *m, const uint64_t *off, size_t mb, size_t n, const void *dst, size_t dl, void *o, void *st) { return hash_dev(1, m, off, mb, n, dst, dl, o, st); }
int gpbc_hash_to_field_dev(const void *m, const uint64_t *off, size_t mb, size_t n, const void *dst, size_t dl, int count, void *o, void *st) {
    if (count != 2 && count != 4) return fail(GPBC_ERR_INVALID_ARG, "count must be 2 or 4");
    return hash_dev(count, m, off, mb, n, dst, dl, o, st);
}

// ----------------------------------------------------------------------------------------------- the XOR mask from GT bytes
int gpbc_mask_version(void) { return 1; }

constexpr size_t MASK_MAX_N = (size_t)0x7fffffff * MASK_BLOCK / MASK_WINDOWS;      // the grid's x extent, twelve lanes per item
int gpbc_gt_xor_mask_dev(const void *d_gt, const void *d_msgs, const uint64_t *d_msg_off, size_t msgs_bytes, size_t width, size_t n, void *d_out,
                         uint32_t *d_out_len, void *stream) {
    if (!n) return GPBC_OK;
    TRY(call_limit("items", n, MASK_MAX_N));
    if (!d_msg_off && width && n > msgs_bytes / width) return fail(GPBC_ERR_INVALID_ARG, "n * width exceeds msgs_bytes (n = %zu, width = %zu, msgs_bytes = %zu)", n, width, msgs_bytes);
    const size_t span = d_msg_off ? msgs_bytes : n * width;        // what the messages, and the output, can occupy
    if (!d_gt || (span && (!d_msgs || !d_out))) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    if (ranges_overlap(d_gt, n * GPBC_GT_BYTES, d_out, span)) return fail(GPBC_ERR_INVALID_ARG, "out overlaps gt");
    TRY(bind_device());
    const int wpi = mask_lanes_per_item(!d_msg_off, width);
    const size_t lanes = d_msg_off ? (n + MASK_GROUP - 1) / MASK_GROUP * MASK_GROUP * MASK_WINDOWS : n * (size_t)wpi;
    return GPBC_LAUNCH(k_gt_xor_mask, (unsigned)((lanes + MASK_BLOCK - 1) / MASK_BLOCK), MASK_BLOCK, (hipStream_t)stream, (const uint8_t *)d_gt,
                       (const uint8_t *)d_msgs, d_msg_off, msgs_bytes, width, n, wpi, (uint8_t *)d_out, d_out_len);
}
// Host pointers: the shared staging path (host_call) through device blocks on the calling thread's current device — the GT rows, the
// bytes the offsets span and the offsets rebased to them travel as whole columns, the kernel runs in place on the device's copy of the
// messages and that copy comes back into `out`; not combined with other threads' calls, not sharded.
int gpbc_gt_xor_mask(const void *gt, const void *msgs, const uint64_t *msg_off, size_t width, size_t n, void *out, uint32_t *out_len) {
    if (!n) return GPBC_OK;
    TRY(call_limit("items", n, MASK_MAX_N));
    if (!gt) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    uint64_t base = 0, bytes = 0;
    std::vector<uint64_t> rel;
    if (msg_off) {
        for (size_t i = 0; i < n; i++) if (msg_off[i + 1] < msg_off[i]) return fail(GPBC_ERR_INVALID_ARG, "message offsets must not decrease");
        base = msg_off[0]; bytes = msg_off[n] - base;
        rel.resize(n + 1);
        for (size_t i = 0; i <= n; i++) rel[i] = msg_off[i] - base;
    } else {
        if (width && n > ~(size_t)0 / width) return fail(GPBC_ERR_INVALID_ARG, "n * width overflows (n = %zu, width = %zu)", n, width);
        bytes = n * width;
    }
    if (bytes && (!msgs || !out)) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    const uint8_t *src = bytes ? (const uint8_t *)msgs + base : nullptr;
    uint8_t *dst = bytes ? (uint8_t *)out + base : nullptr;
    if (ranges_overlap(gt, n * GPBC_GT_BYTES, dst, bytes)) return fail(GPBC_ERR_INVALID_ARG, "out overlaps gt");
    if (out != msgs && ranges_overlap(src, bytes, dst, bytes)) return fail(GPBC_ERR_INVALID_ARG, "out overlaps msgs (only out == msgs runs in place)");
    if (out_len && (ranges_overlap(out_len, n * sizeof(uint32_t), dst, bytes) || ranges_overlap(out_len, n * sizeof(uint32_t), gt, n * GPBC_GT_BYTES)))
        return fail(GPBC_ERR_INVALID_ARG, "out_len overlaps out or gt");
    // ONE unit of whole columns: column 0 is the message bytes and, in place, the output
    HostCall c = HostCall().input(src, bytes, true).input(gt, n * GPBC_GT_BYTES, true);
    if (msg_off) c.input(rel.data(), (n + 1) * sizeof(uint64_t), true);
    c.output(dst, bytes).output(out_len, n * sizeof(uint32_t));
    c.in_place = true;
    return host_call(1, c, HostRoute{}, [&](const DevCols &d, size_t, hipStream_t st) {
        return gpbc_gt_xor_mask_dev(d.in[1], d.in[0], msg_off ? (const uint64_t *)d.in[2] : nullptr, bytes, width, n, d.out[0], (uint32_t *)d.out[1], st);
    });
}

}  // extern "C"
