// ChaCha20 blocks addressed by (seed, stream, index), one block per lane: the randomness of the batched Encrypt / KeyGenerate planners
// made where it is used (csrc/gpbc_hash.hip: k_random_bytes, k_fr_random; include/gpbc_bn254_random.h).  Replaces the caller-side
// fr.SetRandom() of every reference Encrypt and KeyGenerate (cpabe/bsw07/bsw07_cpabe.go, utils/generate_random_polynomial.go,
// fibe/sw05_fibe_common.go:205-210) by a generator whose output at a position depends on nothing but (seed, stream, index).
//
// The block function is RFC 8439 section 2.3 with 20 rounds on the ORIGINAL ChaCha20 state layout: words 0..3 the constants, 4..11 the
// 32-byte seed as little-endian words, 12 and 13 the 64-bit block counter `index` (low word first), 14 and 15 the 64-bit nonce `stream`
// (low word first).  Consecutive indices of one stream are a plain ChaCha20 keystream; the RFC's 2.3.2 vector (32-bit counter 1, nonce
// 00 00 00 09 00 00 00 4a 00 00 00 00) is index 0x0900000000000001 of stream 0x4a000000.
//
// Everything is in 16 named words with constant indices (registers on the device), no table, no data-dependent branch or address.
// Plain C++: the interval harness (tools/bounds_check.cpp: hc_chacha_blocks) compiles this header for the host and holds it against
// the known answers before any kernel runs it.
#ifndef GPBC_CHACHA29_HIP_HPP
#define GPBC_CHACHA29_HIP_HPP
#include "fe29.hip.hpp"

namespace gpbc {

// the seed and the stream as they travel: a kernel argument passed by value, never a buffer
struct ChaChaKey { uint32_t seed[8]; uint32_t stream_lo, stream_hi; };

GPBC_INLINE ChaChaKey chacha_key(const uint8_t *seed32, uint64_t stream) {
    ChaChaKey k;
    for (int i = 0; i < 8; i++)
        k.seed[i] = (uint32_t)seed32[4 * i] | (uint32_t)seed32[4 * i + 1] << 8 | (uint32_t)seed32[4 * i + 2] << 16 | (uint32_t)seed32[4 * i + 3] << 24;
    k.stream_lo = (uint32_t)stream;
    k.stream_hi = (uint32_t)(stream >> 32);
    return k;
}

GPBC_INLINE uint32_t chacha_rotl(uint32_t x, int n) {
#if defined(__has_builtin)
#if __has_builtin(__builtin_rotateleft32)
    return __builtin_rotateleft32(x, (uint32_t)n);
#else
    return (x << n) | (x >> (32 - n));
#endif
#else
    return (x << n) | (x >> (32 - n));
#endif
}
GPBC_INLINE void chacha_quarter(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d) {
    a += b; d ^= a; d = chacha_rotl(d, 16);
    c += d; b ^= c; b = chacha_rotl(b, 12);
    a += b; d ^= a; d = chacha_rotl(d, 8);
    c += d; b ^= c; b = chacha_rotl(b, 7);
}

// out: the 16 words of block `index`; its 64 bytes are the words in order, each little-endian
GPBC_INLINE void chacha20_block(uint32_t (&out)[16], const ChaChaKey &key, uint64_t index) {
    uint32_t in[16];
    in[0] = 0x61707865u; in[1] = 0x3320646eu; in[2] = 0x79622d32u; in[3] = 0x6b206574u;         // "expand 32-byte k"
#pragma unroll
    for (int i = 0; i < 8; i++) in[4 + i] = key.seed[i];
    in[12] = (uint32_t)index; in[13] = (uint32_t)(index >> 32);
    in[14] = key.stream_lo; in[15] = key.stream_hi;
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = in[i];
#pragma unroll
    for (int round = 0; round < 10; round++) {
        chacha_quarter(x[0], x[4], x[8], x[12]);
        chacha_quarter(x[1], x[5], x[9], x[13]);
        chacha_quarter(x[2], x[6], x[10], x[14]);
        chacha_quarter(x[3], x[7], x[11], x[15]);
        chacha_quarter(x[0], x[5], x[10], x[15]);
        chacha_quarter(x[1], x[6], x[11], x[12]);
        chacha_quarter(x[2], x[7], x[8], x[13]);
        chacha_quarter(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = x[i] + in[i];
}

// A lane's 32 or 64 contiguous output bytes, PIECES x 16: one 128-bit store per piece where the address allows it (wide: the buffer
// starts on a 16-byte boundary), byte stores otherwise.  The loads of a 64-byte string likewise.
struct alignas(16) ChaChaPiece { uint32_t w0, w1, w2, w3; };
template <int PIECES> GPBC_INLINE void chacha_store(uint8_t *at, const uint32_t *w, bool wide) {
    if (wide) {
#pragma unroll
        for (int p = 0; p < PIECES; p++) reinterpret_cast<ChaChaPiece *>(at)[p] = ChaChaPiece{w[4 * p], w[4 * p + 1], w[4 * p + 2], w[4 * p + 3]};
    } else {
#pragma unroll
        for (int i = 0; i < 16 * PIECES; i++) at[i] = (uint8_t)(w[i >> 2] >> 8 * (i & 3));
    }
}
GPBC_INLINE void chacha_load64(uint32_t (&w)[16], const uint8_t *at, bool wide) {
    if (wide) {
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const ChaChaPiece q = reinterpret_cast<const ChaChaPiece *>(at)[p];
            w[4 * p] = q.w0; w[4 * p + 1] = q.w1; w[4 * p + 2] = q.w2; w[4 * p + 3] = q.w3;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = (uint32_t)at[4 * i] | (uint32_t)at[4 * i + 1] << 8 | (uint32_t)at[4 * i + 2] << 16 | (uint32_t)at[4 * i + 3] << 24;
    }
}

}  // namespace gpbc
#endif
