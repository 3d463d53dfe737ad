// libgpbc_bn254.so, one of the units listed in _build.py: SHA-256 on the device with the digest as bytes or as a scalar — the transcript hash H(u, v, w) of
// Gentry06 and the plain batched SHA-256 (csrc/transcript29.hip.hpp) with their C-ABI entries (include/gpbc_bn254_hash.h); and, as the
// byte unit that already has Fr, the seed-addressed generator — ChaCha20 blocks and their reduction into Fr (csrc/chacha29.hip.hpp,
// fr_wide_reduce) — with the entries of include/gpbc_bn254_random.h.  gfx950 only.
#include "gpbc_common.hpp"
#include "../../include/gpbc_bn254_hash.h"
#include "../../include/gpbc_bn254_random.h"
#include "transcript29.hip.hpp"
#include "chacha29.hip.hpp"

// one item per lane: 832 bytes in, 32 out
GPBC_KERNEL_G1 k_hash_g1_gt_gt_to_fr(const uint8_t *__restrict__ u, const uint8_t *__restrict__ v, const uint8_t *__restrict__ w, size_t n, uint8_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    hash_g1_gt_gt_to_fr_lane(u + i * GPBC_G1_BYTES, v + i * GPBC_GT_BYTES, w + i * GPBC_GT_BYTES, out + i * GPBC_SCALAR_BYTES);
}
// one message per lane: message i is msgs[off[i], off[i+1]), the offsets clamped as the hash-to-curve kernels clamp them (msg_range)
GPBC_KERNEL_G1 k_sha256(const uint8_t *__restrict__ msgs, const uint64_t *__restrict__ off, size_t total, size_t n, int to_fr, uint8_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint64_t lo, len;
    msg_range(off, total, i, lo, len);
    sha256_lane(msgs + lo, len, to_fr != 0, out + i * 32);
}
// one block per lane: lane i makes block first + i of the stream (a 64-bit add) and writes its 64 bytes, or the 32 of the scalar they
// reduce to.  The seed and the stream are the by-value argument `key`; wide: out is on a 16-byte boundary.
GPBC_KERNEL_G1 k_random_bytes(ChaChaKey key, uint64_t first, size_t n, int wide, uint8_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t w[16];
    chacha20_block(w, key, first + i);
    chacha_store<4>(out + i * GPBC_RANDOM_BLOCK_BYTES, w, wide != 0);
}
GPBC_KERNEL_G1 k_fr_random(ChaChaKey key, uint64_t first, size_t n, int wide, uint8_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t w[16], s[8];
    chacha20_block(w, key, first + i);
    fr_words(s, fr_wide_reduce(w));
    chacha_store<2>(out + i * GPBC_SCALAR_BYTES, s, wide != 0);
}
// one 64-byte string per lane, in and out each wide or not by its own address
GPBC_KERNEL_G1 k_fr_set_bytes64(const uint8_t *__restrict__ in, size_t n, int wide_in, int wide_out, uint8_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t w[16], s[8];
    chacha_load64(w, in + i * GPBC_RANDOM_BLOCK_BYTES, wide_in != 0);
    fr_words(s, fr_wide_reduce(w));
    chacha_store<2>(out + i * GPBC_SCALAR_BYTES, s, wide_out != 0);
}

// what every entry of the generator refuses before it touches a device: the message names the argument, never a seed byte
constexpr size_t RANDOM_MAX_N = (size_t)0x7fffffff * BLOCK;                  // the grid's x extent
static int random_args(const void *seed, size_t first, size_t n, const void *out) {
    if (!seed || !out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    if (first && n > (size_t)0 - first) return fail(GPBC_ERR_INVALID_ARG, "first + n exceeds 2^64 (first = %zu, n = %zu)", first, n);
    return call_limit("elements", n, RANDOM_MAX_N);
}
static bool wide_at(const void *p) { return ((uintptr_t)p & 15) == 0; }

extern "C" {

int gpbc_hash_version(void) { return 1; }
int gpbc_random_version(void) { return 1; }

int gpbc_random_bytes_dev(const void *seed, size_t stream, size_t first, size_t n_blocks, void *d_out, void *hip_stream) {
    if (!n_blocks) return GPBC_OK;
    TRY(random_args(seed, first, n_blocks, d_out));
    TRY(bind_device());
    return GPBC_LAUNCH(k_random_bytes, grid_for(n_blocks), BLOCK, (hipStream_t)hip_stream, chacha_key((const uint8_t *)seed, stream), (uint64_t)first, n_blocks,
                       (int)wide_at(d_out), (uint8_t *)d_out);
}
// Host pointers: the shared staging path (host_call) with no input column — a device block for the output on the calling thread's
// current device, the launch on the null stream, one download; not combined with other threads' calls, not sharded.
int gpbc_random_bytes(const void *seed, size_t stream, size_t first, size_t n_blocks, void *out) {
    if (!n_blocks) return GPBC_OK;
    TRY(random_args(seed, first, n_blocks, out));
    return host_call(n_blocks, HostCall().output(out, GPBC_RANDOM_BLOCK_BYTES), HostRoute{},
                     [&](const DevCols &d, size_t m, hipStream_t st) { return gpbc_random_bytes_dev(seed, stream, first, m, d.out[0], st); });
}
int gpbc_fr_random_dev(const void *seed, size_t stream, size_t first, size_t n, void *d_out, void *hip_stream) {
    if (!n) return GPBC_OK;
    TRY(random_args(seed, first, n, d_out));
    TRY(bind_device());
    return GPBC_LAUNCH(k_fr_random, grid_for(n), BLOCK, (hipStream_t)hip_stream, chacha_key((const uint8_t *)seed, stream), (uint64_t)first, n, (int)wide_at(d_out),
                       (uint8_t *)d_out);
}
int gpbc_fr_random(const void *seed, size_t stream, size_t first, size_t n, void *out) {
    if (!n) return GPBC_OK;
    TRY(random_args(seed, first, n, out));
    return host_call(n, HostCall().output(out, GPBC_SCALAR_BYTES), HostRoute{},
                     [&](const DevCols &d, size_t m, hipStream_t st) { return gpbc_fr_random_dev(seed, stream, first, m, d.out[0], st); });
}
static int set_bytes64_args(const void *in, size_t n, const void *out) {
    if (!in || !out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    TRY(call_limit("elements", n, RANDOM_MAX_N));
    if (ranges_overlap(in, n * GPBC_RANDOM_BLOCK_BYTES, out, n * GPBC_SCALAR_BYTES)) return fail(GPBC_ERR_INVALID_ARG, "out overlaps in");
    return GPBC_OK;
}
int gpbc_fr_set_bytes64_dev(const void *d_in, size_t n, void *d_out, void *hip_stream) {
    if (!n) return GPBC_OK;
    TRY(set_bytes64_args(d_in, n, d_out));
    TRY(bind_device());
    return GPBC_LAUNCH(k_fr_set_bytes64, grid_for(n), BLOCK, (hipStream_t)hip_stream, (const uint8_t *)d_in, n, (int)wide_at(d_in), (int)wide_at(d_out), (uint8_t *)d_out);
}
int gpbc_fr_set_bytes64(const void *in, size_t n, void *out) {
    if (!n) return GPBC_OK;
    TRY(set_bytes64_args(in, n, out));
    return host_call(n, HostCall().input(in, GPBC_RANDOM_BLOCK_BYTES).output(out, GPBC_SCALAR_BYTES), HostRoute{},
                     [](const DevCols &d, size_t m, hipStream_t st) { return gpbc_fr_set_bytes64_dev(d.in[0], m, d.out[0], st); });
}

int gpbc_sha256_batch_dev(const void *d_msgs, const uint64_t *d_msg_off, size_t msgs_bytes, size_t n, int to_fr, void *d_out, void *stream) {
    if (!n) return GPBC_OK;
    if (!d_msg_off || !d_out || (msgs_bytes && !d_msgs)) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    TRY(bind_device());
    return GPBC_LAUNCH(k_sha256, grid_for(n), BLOCK, (hipStream_t)stream, (const uint8_t *)d_msgs, d_msg_off, msgs_bytes, n, to_fr, (uint8_t *)d_out);
}
// Host pointers: the shared staging path (host_call) through device blocks on the calling thread's current device — the messages the
// offsets span and the offsets rebased to them travel as whole columns; not combined with other threads' calls, not sharded.
int gpbc_sha256_batch(const void *msgs, const uint64_t *msg_off, size_t n, int to_fr, void *out) {
    if (!n) return GPBC_OK;
    if (!msg_off || !out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    for (size_t i = 0; i < n; i++) if (msg_off[i + 1] < msg_off[i]) return fail(GPBC_ERR_INVALID_ARG, "message offsets must not decrease");
    const uint64_t base = msg_off[0], bytes = msg_off[n] - base;
    if (bytes && !msgs) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    std::vector<uint64_t> rel(n + 1);
    for (size_t i = 0; i <= n; i++) rel[i] = msg_off[i] - base;
    HostCall c = HostCall().input(bytes ? (const uint8_t *)msgs + base : nullptr, bytes, true).input(rel.data(), (n + 1) * sizeof(uint64_t), true).output(out, 32);
    return host_call(n, c, HostRoute{}, [&](const DevCols &d, size_t m, hipStream_t st) {
        return gpbc_sha256_batch_dev(d.in[0], (const uint64_t *)d.in[1], bytes, m, to_fr, d.out[0], st);
    });
}

int gpbc_hash_g1_gt_gt_to_fr_dev(const void *d_u, const void *d_v, const void *d_w, size_t n, void *d_out, void *stream) {
    if (!n) return GPBC_OK;
    if (!d_u || !d_v || !d_w || !d_out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    TRY(bind_device());
    return GPBC_LAUNCH(k_hash_g1_gt_gt_to_fr, grid_for(n), BLOCK, (hipStream_t)stream, (const uint8_t *)d_u, (const uint8_t *)d_v, (const uint8_t *)d_w, n, (uint8_t *)d_out);
}
int gpbc_hash_g1_gt_gt_to_fr(const void *u, const void *v, const void *w, size_t n, void *out) {
    if (!n) return GPBC_OK;
    if (!u || !v || !w || !out) return fail(GPBC_ERR_INVALID_ARG, "null pointer");
    return host_call(n, HostCall().input(u, GPBC_G1_BYTES).input(v, GPBC_GT_BYTES).input(w, GPBC_GT_BYTES).output(out, GPBC_SCALAR_BYTES), HostRoute{},
                     [](const DevCols &d, size_t m, hipStream_t st) { return gpbc_hash_g1_gt_gt_to_fr_dev(d.in[0], d.in[1], d.in[2], m, d.out[0], st); });
}

}  // extern "C"
