// The XOR mask from GT bytes: out_i = msg_i XOR GT.Bytes()(gt_i), cut to the shorter operand — the last step of Boneh-Franklin
// BasicIdent Encrypt and Decrypt (reference ibe/bf01_ibe/bf01_ibe.go:170-176,202-208: utils.Xor(message, hash.FromGT(gid));
// hash/hash_from_gt.go:5-8, utils/xor.go:3-16).  B = GT.Bytes() is 384 bytes, the twelve coefficients as big-endian canonical
// integers from C1.B2.A1 down to C0.B0.A0 (wire29.hip.hpp): byte window w, bytes 32 w .. 32 w + 31 of B, is coefficient 11 - w of the
// in-memory order.
//
// One lane per (item, window), `wpi` lanes per item: twelve where the lengths are in device memory (the offset form), and in the row
// form as many as a row of `width` bytes has windows, min(12, ceil(width / 32)) — known on the host, so the lanes that could only
// exit are not launched (a wavefront in which one lane of twelve converts costs what one in which all do costs: 2^20 rows of 32 bytes
// took 0.292 ms with twelve lanes per item and take 0.036 ms with one).  With len the length of message i and
// L = min(len, 384):
//     out[j] = msg[j] ^ B[j]   0 <= j < L          out[j] = 0   L <= j < len          out_len = L
// A lane whose window starts at or past L never loads or converts its coefficient: a 32-byte message costs one conversion out of
// Montgomery form, not twelve, and the lanes of an item read adjacent 32-byte pieces of its GT row.  The tail past 384 bytes (it
// exists only where wpi = 12) is zeroed in 32-byte pieces dealt round the same twelve lanes (piece 12 + w, 24 + w, ... to lane w), so
// lane w touches exactly the pieces w, w + 12, ... of its own item and nothing else: no byte of another item is read or written
// whatever the offsets.
// Pieces go as two 16-byte or eight 4-byte accesses where the piece is whole and both addresses allow, byte by byte otherwise (an odd
// offset, the partly used last piece).  In place (out == msgs, the identical pointer): a lane loads all bytes of a piece before it
// stores any, and every output byte is written by the lane that read the message byte at that address.  No LDS; lengths and
// addresses are public and the only things branched on — the conversion (fe_to_plain_words) is the wire formats' own.
#ifndef GPBC_MASK29_HIP_HPP
#define GPBC_MASK29_HIP_HPP
#include "wire29.hip.hpp"
#include "xmd29.hip.hpp"

namespace gpbc {

constexpr int MASK_BLOCK = 256;                 // lanes per workgroup: 21 items and a third at twelve lanes per item
constexpr int MASK_PIECE = 32, MASK_WINDOWS = 12;
constexpr uint64_t MASK_BYTES = 384;

// window w of GT.Bytes() of the element at `gt` as eight words in memory order (word k = bytes 4 k .. 4 k + 3 of the window)
__device__ __forceinline__ void mask_window_words(uint32_t (&m)[8], const uint8_t *__restrict__ gt, int w) {
    uint32_t p[8];
    fe_to_plain_words(p, fe_load(gt + 32 * (MASK_WINDOWS - 1 - w)));
#pragma unroll
    for (int k = 0; k < 8; k++) m[k] = wire_bswap(p[7 - k]);
}

// q[0, cnt) = p[0, cnt) ^ the window's first cnt bytes, 1 <= cnt <= 32; q == p is allowed (loads before stores)
__device__ __forceinline__ void mask_xor_piece(uint8_t *q, const uint8_t *p, const uint32_t (&m)[8], int cnt) {
    const uintptr_t both = (uintptr_t)p | (uintptr_t)q;
    if (cnt == MASK_PIECE && !(both & 15)) {
        uint4 a = reinterpret_cast<const uint4 *>(p)[0], b = reinterpret_cast<const uint4 *>(p)[1];
        a.x ^= m[0]; a.y ^= m[1]; a.z ^= m[2]; a.w ^= m[3];
        b.x ^= m[4]; b.y ^= m[5]; b.z ^= m[6]; b.w ^= m[7];
        reinterpret_cast<uint4 *>(q)[0] = a;
        reinterpret_cast<uint4 *>(q)[1] = b;
    } else if (cnt == MASK_PIECE && !(both & 3)) {
        uint32_t v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = reinterpret_cast<const uint32_t *>(p)[k];
#pragma unroll
        for (int k = 0; k < 8; k++) reinterpret_cast<uint32_t *>(q)[k] = v[k] ^ m[k];
    } else {
        uint32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};                // the piece's bytes packed as the words above pack them
#pragma unroll
        for (int j = 0; j < MASK_PIECE; j++) if (j < cnt) v[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
#pragma unroll
        for (int j = 0; j < MASK_PIECE; j++) if (j < cnt) q[j] = (uint8_t)((v[j >> 2] ^ m[j >> 2]) >> (8 * (j & 3)));
    }
}
// q[0, cnt) = 0, 1 <= cnt <= 32
__device__ __forceinline__ void mask_zero_piece(uint8_t *q, int cnt) {
    if (cnt == MASK_PIECE && !((uintptr_t)q & 15)) {
        reinterpret_cast<uint4 *>(q)[0] = uint4{0, 0, 0, 0};
        reinterpret_cast<uint4 *>(q)[1] = uint4{0, 0, 0, 0};
    } else if (cnt == MASK_PIECE && !((uintptr_t)q & 3)) {
#pragma unroll
        for (int k = 0; k < 8; k++) reinterpret_cast<uint32_t *>(q)[k] = 0;
    } else {
#pragma unroll
        for (int j = 0; j < MASK_PIECE; j++) if (j < cnt) q[j] = 0;
    }
}

// The offset form's lane order: items in groups of MASK_GROUP = 64, a group's 768 lanes window-major — wavefront w of the group is
// window w of its 64 items (a workgroup of 256 lanes is four such wavefronts; 768 = 3 workgroups).  Lengths are not known on the host
// there, but short messages leave whole wavefronts idle, and an idle wavefront costs two offset loads where an idle lane beside busy
// ones costs the whole conversion.  Neighbouring lanes then read 32-byte pieces 384 bytes apart in gt; the pieces between them go to
// the group's other wavefronts.
constexpr int MASK_GROUP = 64;
__device__ __forceinline__ void mask_ragged_lane(size_t lane, size_t &i, int &w) {
    const size_t group = lane / (MASK_GROUP * MASK_WINDOWS), r = lane - group * (MASK_GROUP * MASK_WINDOWS);
    w = (int)(r / MASK_GROUP);
    i = group * MASK_GROUP + (r - (size_t)w * MASK_GROUP);
}

// lanes per item of a call: every window a message of the call can reach
inline int mask_lanes_per_item(bool rows, size_t width) {
    if (!rows || width > (size_t)MASK_PIECE * (MASK_WINDOWS - 1)) return MASK_WINDOWS;
    return width <= MASK_PIECE ? 1 : (int)((width + MASK_PIECE - 1) / MASK_PIECE);
}

// Lane w < wpi of item i.  off != null: message i is msgs[off[i], off[i + 1]) with the offsets clamped to [0, total] and the length to
// >= 0 (msg_range, xmd29.hip.hpp), wpi = 12; off == null: rows of `width` bytes (the caller has checked n * width <= total),
// wpi = mask_lanes_per_item.  out has the layout of msgs; out_len may be null.
__device__ __forceinline__ void gt_xor_mask_lane(const uint8_t *__restrict__ gt, const uint8_t *msgs, const uint64_t *off, size_t total, size_t width,
                                                 size_t i, int w, uint8_t *out, uint32_t *out_len) {
    uint64_t lo, len;
    if (off) msg_range(off, total, i, lo, len);
    else { lo = (uint64_t)i * width; len = width; }
    const uint64_t L = len < MASK_BYTES ? len : MASK_BYTES, at = (uint64_t)MASK_PIECE * w;
    if (w == 0 && out_len) out_len[i] = (uint32_t)L;
    if (at >= L) return;                                         // (at < 384, so this is also at >= len: no tail piece either)
    uint32_t m[8];
    mask_window_words(m, gt + i * MASK_BYTES, w);
    const uint64_t left = L - at;
    mask_xor_piece(out + lo + at, msgs + lo + at, m, left < MASK_PIECE ? (int)left : MASK_PIECE);
    for (uint64_t t = at + MASK_BYTES; t < len; t += MASK_BYTES) {
        const uint64_t rest = len - t;
        mask_zero_piece(out + lo + t, rest < MASK_PIECE ? (int)rest : MASK_PIECE);
    }
}

}  // namespace gpbc
#endif
