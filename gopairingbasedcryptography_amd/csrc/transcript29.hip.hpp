// SHA-256 of group elements and of plain messages, one item per lane, with the digest taken as a scalar — the hash in the middle of
// the CCA-secure Gentry06 IBE (ibe/gentry06_ibe/gentry06_ibe.go:319-343):
//     beta = H(u, v, w) = fr.SetBytes(SHA-256(u.Bytes() || v.Bytes() || w.Bytes())),   u in G1 (compressed form), v, w in GT
// and the plain SHA-256 of NewWaters05IBEIdentity / NewBB04IBEIdentity.  Joins the register-resident compression of xmd29.hip.hpp, the
// canonical encodings of wire29.hip.hpp and the canonical reduction of fr29.hip.hpp.
//
// The transcript is 800 bytes = 25 big-endian 32-byte coordinates: u.X with the compressed-form flag in its two top bits (coordinate 0),
// the twelve coefficients of v in wire order C1.B2.A1 ... C0.B0.A0 (1..12), the twelve of w (13..24).  It fills 13 blocks: block b < 12
// is coordinates 2b and 2b + 1; block 12 is coordinate 24, then 0x80, zeros and the 64-bit length 6400.  A coordinate's eight message
// words are its canonical plain words (fe_load -> fe_to_plain_words, least significant first) in reverse order, so no byte is handled and
// the 800 bytes exist nowhere: a lane holds the eight chaining words, the sixteen words of the block it is filling and one coordinate
// conversion.  Edge inputs as g1_wire_encode / gt_wire_encode treat them: the all-zero u is infinity and hashes as 0x40 and 31 zero
// bytes, the Y flag is 0x80 / 0xC0 by fe_lex_largest(y); GT elements are encoded as they are (no membership test).
//
// Digest -> scalar: the eight digest words, most significant first as SHA-256 leaves them, are the integer's words in reverse; that
// integer (below 2^256) goes through the scalar format's own load, reduction and canonical store (fr_load_raw, fr_reduce,
// fr_canonical, fr_store_canonical), so the output is the canonical residue in [0, r) every scalar argument of the ABI takes.
#ifndef GPBC_TRANSCRIPT29_HIP_HPP
#define GPBC_TRANSCRIPT29_HIP_HPP
#include "xmd29.hip.hpp"
#include "fr29.hip.hpp"

namespace gpbc {

constexpr int TRANSCRIPT_COORDS = 25, TRANSCRIPT_BYTES = 32 * TRANSCRIPT_COORDS;

// fr.Element.SetBytes(digest) in the scalar format: out = the digest as a big-endian integer, mod r
GPBC_INLINE void sha256_digest_to_fr(uint8_t *out, const uint32_t (&st)[8]) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = st[7 - i];
    const Fr x = fr_load_raw(reinterpret_cast<const uint8_t *>(w));
    fr_store_canonical(out, fr_canonical<1, 2>(fr_reduce(x)));
}
// the 32 digest bytes as SHA-256 writes them
GPBC_INLINE void sha256_digest_store(uint8_t *out, const uint32_t (&st)[8]) {
    uint32_t *q = reinterpret_cast<uint32_t *>(out);
#pragma unroll
    for (int i = 0; i < 8; i++) q[i] = wire_bswap(st[i]);
}

// the eight message words of one coordinate: the gnark fp.Element at p, `first_or` into the top bits of its first byte
GPBC_INLINE void transcript_coord(uint32_t *m, const uint8_t *p, uint32_t first_or) {
    uint32_t w[8];
    fe_to_plain_words(w, fe_load(p));
#pragma unroll
    for (int j = 0; j < 8; j++) m[j] = w[7 - j];
    m[0] |= first_or << 24;
}
// coordinate k of the transcript, 1 <= k <= 24: GT coefficient 11 - q of the memory order sits at wire position q
GPBC_INLINE const uint8_t *transcript_gt_coord(const uint8_t *v, const uint8_t *w, int k) {
    return k <= 12 ? v + 32 * (12 - k) : w + 32 * (24 - k);
}

// beta = H(u, v, w): u one gnark G1Affine (64 B), v and w gnark GT (384 B each), out one scalar (32 B)
GPBC_INLINE void hash_g1_gt_gt_to_fr_lane(const uint8_t *u, const uint8_t *v, const uint8_t *w, uint8_t *out) {
    uint32_t st[8], m[16];
    sha256_iv(st);
    if (bytes_all_zero(u, 16)) {
#pragma unroll
        for (int j = 0; j < 8; j++) m[j] = j == 0 ? (uint32_t)WIRE_INFINITY << 24 : 0u;
    } else {
        transcript_coord(m, u, fe_lex_largest(fe_load(u + 32)) ? WIRE_LARGEST : WIRE_SMALLEST);
    }
    transcript_coord(m + 8, transcript_gt_coord(v, w, 1), 0);
    sha256_compress(st, m);
    for (int b = 1; b < 12; b++) {
        transcript_coord(m, transcript_gt_coord(v, w, 2 * b), 0);
        transcript_coord(m + 8, transcript_gt_coord(v, w, 2 * b + 1), 0);
        sha256_compress(st, m);
    }
    transcript_coord(m, transcript_gt_coord(v, w, 24), 0);
#pragma unroll
    for (int j = 8; j < 16; j++) m[j] = j == 8 ? 0x80000000u : j == 15 ? 8u * TRANSCRIPT_BYTES : 0u;
    sha256_compress(st, m);
    sha256_digest_to_fr(out, st);
}

// SHA-256 of one message: the 32 digest bytes, or (to_fr) the digest as a scalar
GPBC_INLINE void sha256_lane(const uint8_t *msg, uint64_t len, bool to_fr, uint8_t *out) {
    uint32_t st[8];
    sha256_iv(st);
    sha256_tail<0>(st, 0, len, [&](uint64_t pos) -> uint32_t { return msg[pos]; });
    if (to_fr) sha256_digest_to_fr(out, st);
    else sha256_digest_store(out, st);
}

}  // namespace gpbc
#endif
