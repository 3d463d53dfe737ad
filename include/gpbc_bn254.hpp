// gpbc_bn254.hpp — header-only C++ mirror of the gnark-crypto bn254 surface the reference calls, over the C ABI
// (gpbc_bn254.h).  Same names, argument meaning and error behaviour as the Go API:
//
//   bn254.Pair(P []G1Affine, Q []G2Affine) (GT, error)          -> bn254::Pair(P, Q)            throws on size mismatch
//   bn254.PairingCheck(P, Q) (bool, error)                      -> bn254::PairingCheck(P, Q)
//   new(G1Affine).ScalarMultiplication(&a, s)                   -> G1Affine().ScalarMultiplication(a, s)
//   new(G1Affine).ScalarMultiplicationBase(s)                   -> G1Affine().ScalarMultiplicationBase(s)
//   new(GT).Exp(x, k) / Mul / Div / Inverse                     -> GT().Exp(x, k) ...
//   bn254.Generators()                                          -> bn254::Generators()
//   p.Marshal() / p.Bytes() / p.Unmarshal(buf)  (G1, G2, GT)    -> same names; Unmarshal throws where gnark errors
//
// Structs have gnark's in-memory layout (fp.Element = 4 LE u64 Montgomery limbs), so arrays of them are the ABI
// buffers.  Scalars are `Scalar` = 32-byte little-endian plain integers (what the cgo shim makes of *big.Int).
// The Go toolchain is absent from the build image; this header is the compiled-language host side used by
// tests/cpp/ (reference is Go, see INTEGRATION.md for the cgo shim).
#ifndef GPBC_BN254_HPP
#define GPBC_BN254_HPP
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "gpbc_bn254.h"
#include "gpbc_bn254_hash.h"
#include "gpbc_bn254_share.h"
#include "gpbc_bn254_indexed.h"
#include "gpbc_bn254_select.h"

namespace bn254 {

struct Scalar {
    std::array<uint8_t, 32> le{};
    Scalar() = default;
    explicit Scalar(uint64_t v) { for (int i = 0; i < 8; i++) le[i] = (uint8_t)(v >> (8 * i)); }
};

inline void check(int rc) { if (rc < 0) throw std::runtime_error(std::string("gpbc: ") + gpbc_last_error()); }
inline void Init(int device = 0) { check(gpbc_init(device)); }
// Bind the process to several MI355X (HIP ordinals): host-pointer batch calls then shard over all of them, and a thread
// picks the device of its *_dev calls with SetDevice(index).  InitAllDevices() takes every visible device.
inline void Init(const std::vector<int> &devices) { check(gpbc_init_devices(devices.data(), (int)devices.size())); }
inline int InitAllDevices() {
    int n = gpbc_device_count();
    check(n);
    std::vector<int> d(n);
    for (int i = 0; i < n; i++) d[i] = i;
    Init(d);
    return n;
}
inline int NumDevices() { return gpbc_num_devices(); }
inline void SetDevice(int index) { check(gpbc_set_device(index)); }

struct fpElement { uint64_t l[4]; };
struct E2 { fpElement A0, A1; };

struct G1Affine {
    fpElement X{}, Y{};
    bool IsInfinity() const { uint64_t o = 0; for (int i = 0; i < 4; i++) o |= X.l[i] | Y.l[i]; return o == 0; }
    bool Equal(const G1Affine &b) const { return std::memcmp(this, &b, sizeof *this) == 0; }
    G1Affine &Neg(const G1Affine &a);
    G1Affine &ScalarMultiplication(const G1Affine &a, const Scalar &s) {
        check(gpbc_g1_scalar_mul_batch(&a, 1, s.le.data(), 1, this));
        return *this;
    }
    G1Affine &ScalarMultiplicationBase(const Scalar &s);
    // wire formats (gnark marshal.go): RawBytes 64 B, Bytes 32 B compressed; Unmarshal = SetBytes, returns bytes read
    std::vector<uint8_t> Marshal() const { std::vector<uint8_t> b(GPBC_G1_RAW_BYTES); check(gpbc_g1_marshal_batch(this, 1, 0, b.data())); return b; }
    std::array<uint8_t, GPBC_G1_COMPRESSED_BYTES> Bytes() const { std::array<uint8_t, GPBC_G1_COMPRESSED_BYTES> b; check(gpbc_g1_marshal_batch(this, 1, 1, b.data())); return b; }
    size_t Unmarshal(const std::vector<uint8_t> &buf) {
        if (buf.size() < GPBC_G1_COMPRESSED_BYTES) throw std::invalid_argument("short buffer");
        size_t eb = buf.size() >= GPBC_G1_RAW_BYTES ? GPBC_G1_RAW_BYTES : GPBC_G1_COMPRESSED_BYTES;
        uint8_t ok = 0;
        check(gpbc_g1_unmarshal_batch(buf.data(), eb, 1, this, &ok));
        if (!ok) throw std::invalid_argument("invalid G1 encoding");
        return (buf[0] & 0x80) || (buf[0] & 0xC0) == 0x40 ? GPBC_G1_COMPRESSED_BYTES : GPBC_G1_RAW_BYTES;
    }
};
// host-side field negation p - y on Montgomery limbs (gnark's G1Affine.Neg / G2Affine.Neg; not a hot-path operation)
inline fpElement fpNeg(const fpElement &y) {
    static const uint64_t P[4] = {0x3c208c16d87cfd47ULL, 0x97816a916871ca8dULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
    if ((y.l[0] | y.l[1] | y.l[2] | y.l[3]) == 0) return y;
    fpElement r;
    unsigned __int128 b = 0;
    for (int i = 0; i < 4; i++) {
        unsigned __int128 d = (unsigned __int128)P[i] - y.l[i] - b;
        r.l[i] = (uint64_t)d;
        b = (d >> 64) & 1;
    }
    return r;
}
struct G2Affine {
    E2 X{}, Y{};
    bool Equal(const G2Affine &b) const { return std::memcmp(this, &b, sizeof *this) == 0; }
    G2Affine &Neg(const G2Affine &a) { X = a.X; Y.A0 = fpNeg(a.Y.A0); Y.A1 = fpNeg(a.Y.A1); return *this; }
    G2Affine &ScalarMultiplication(const G2Affine &a, const Scalar &s) {
        check(gpbc_g2_scalar_mul_batch(&a, 1, s.le.data(), 1, this));
        return *this;
    }
    G2Affine &ScalarMultiplicationBase(const Scalar &s);
    std::vector<uint8_t> Marshal() const { std::vector<uint8_t> b(GPBC_G2_RAW_BYTES); check(gpbc_g2_marshal_batch(this, 1, 0, b.data())); return b; }
    std::array<uint8_t, GPBC_G2_COMPRESSED_BYTES> Bytes() const { std::array<uint8_t, GPBC_G2_COMPRESSED_BYTES> b; check(gpbc_g2_marshal_batch(this, 1, 1, b.data())); return b; }
    size_t Unmarshal(const std::vector<uint8_t> &buf) {          // includes gnark's subgroup check
        if (buf.size() < GPBC_G2_COMPRESSED_BYTES) throw std::invalid_argument("short buffer");
        size_t eb = buf.size() >= GPBC_G2_RAW_BYTES ? GPBC_G2_RAW_BYTES : GPBC_G2_COMPRESSED_BYTES;
        uint8_t ok = 0;
        check(gpbc_g2_unmarshal_batch(buf.data(), eb, 1, this, &ok));
        if (!ok) throw std::invalid_argument("invalid G2 encoding");
        return (buf[0] & 0x80) || (buf[0] & 0xC0) == 0x40 ? GPBC_G2_COMPRESSED_BYTES : GPBC_G2_RAW_BYTES;
    }
};
struct GT {
    E2 c[6]{};   // C0.B0, C0.B1, C0.B2, C1.B0, C1.B1, C1.B2
    bool Equal(const GT &b) const { return std::memcmp(this, &b, sizeof *this) == 0; }
    GT &Exp(const GT &x, const Scalar &k) { check(gpbc_gt_exp_batch(&x, k.le.data(), 1, this)); return *this; }
    GT &Mul(const GT &a, const GT &b) { check(gpbc_gt_mul_batch(&a, &b, 1, this)); return *this; }
    GT &Div(const GT &a, const GT &b) { check(gpbc_gt_div_batch(&a, &b, 1, this)); return *this; }
    GT &Inverse(const GT &a) { check(gpbc_gt_inverse_batch(&a, 1, this)); return *this; }
    std::array<uint8_t, GPBC_GT_BYTES> Bytes() const { std::array<uint8_t, GPBC_GT_BYTES> b; check(gpbc_gt_marshal_batch(this, 1, b.data())); return b; }
    std::vector<uint8_t> Marshal() const { auto b = Bytes(); return std::vector<uint8_t>(b.begin(), b.end()); }
    void Unmarshal(const std::vector<uint8_t> &buf) {
        if (buf.size() < GPBC_GT_BYTES) throw std::invalid_argument("short buffer");
        uint8_t ok = 0;
        check(gpbc_gt_unmarshal_batch(buf.data(), 1, this, &ok));
        if (!ok) throw std::invalid_argument("invalid GT encoding");
    }
};
static_assert(sizeof(G1Affine) == GPBC_G1_BYTES && sizeof(G2Affine) == GPBC_G2_BYTES && sizeof(GT) == GPBC_GT_BYTES, "gnark layouts");

// g1 = (1, 2), g2 = the alt_bn128 twist generator, Montgomery form (tools/gen_constants.py values)
inline void Generators(G1Affine &g1, G2Affine &g2) {
    g1.X = {{0xd35d438dc58f0d9dULL, 0x0a78eb28f5c70b3dULL, 0x666ea36f7879462cULL, 0x0e0a77c19a07df2fULL}};
    g1.Y = {{0xa6ba871b8b1e1b3aULL, 0x14f1d651eb8e167bULL, 0xccdd46def0f28c58ULL, 0x1c14ef83340fbe5eULL}};
    g2.X.A0 = {{0x8e83b5d102bc2026ULL, 0xdceb1935497b0172ULL, 0xfbb8264797811adfULL, 0x19573841af96503bULL}};
    g2.X.A1 = {{0xafb4737da84c6140ULL, 0x6043dd5a5802d8c4ULL, 0x09e950fc52a02f86ULL, 0x14fef0833aea7b6bULL}};
    g2.Y.A0 = {{0x619dfa9d886be9f6ULL, 0xfe7fd297f59e9b78ULL, 0xff9e1a62231b7dfeULL, 0x28fd7eebae9e4206ULL}};
    g2.Y.A1 = {{0x64095b56c71856eeULL, 0xdc57f922327d3cbbULL, 0x55f935be33351076ULL, 0x0da4a0e693fd6482ULL}};
}
inline G1Affine &G1Affine::Neg(const G1Affine &a) { X = a.X; Y = fpNeg(a.Y); return *this; }
// ScalarMultiplicationBase: fixed-base window tables of the two generators (1 MB / 2 MB of HBM), built on the first call and
// kept for the life of the process — 32 mixed additions per multiplication instead of the variable-base kernel's doublings.
namespace detail {
struct GeneratorTables {
    gpbc_fixed_base *g1 = nullptr, *g2 = nullptr;
    GeneratorTables() {
        G1Affine a; G2Affine b; Generators(a, b);
        check(gpbc_g1_fixed_base_create(&a, 1, &g1));
        check(gpbc_g2_fixed_base_create(&b, 1, &g2));
    }
};
inline const GeneratorTables &generator_tables() { static const GeneratorTables t; return t; }   // C++11: initialised once, thread-safe
}  // namespace detail
inline G1Affine &G1Affine::ScalarMultiplicationBase(const Scalar &s) { check(gpbc_fixed_base_msm(detail::generator_tables().g1, s.le.data(), 1, this)); return *this; }
inline G2Affine &G2Affine::ScalarMultiplicationBase(const Scalar &s) { check(gpbc_fixed_base_msm(detail::generator_tables().g2, s.le.data(), 1, this)); return *this; }

// prod_i x[i]^k[i] in one call (the Exp + Mul loops of dabe/lw11_dabe.go:180-196, access/tree/access_tree_node.go:123,156) and the
// plain product (gka/agka09/asbb.go:193-207); no factors give one.
inline GT GTMultiExp(const std::vector<GT> &x, const std::vector<Scalar> &k) {
    if (x.size() != k.size()) throw std::invalid_argument("invalid inputs sizes");
    std::vector<uint8_t> e(32 * k.size());
    for (size_t i = 0; i < k.size(); i++) std::memcpy(e.data() + 32 * i, k[i].le.data(), 32);
    const uint64_t seg[2] = {0, x.size()};
    GT z;
    check(gpbc_gt_multi_exp(x.data(), e.data(), k.size(), seg, 1, &z));
    return z;
}
inline GT GTProd(const std::vector<GT> &x) {
    const uint64_t seg[2] = {0, x.size()};
    GT z;
    check(gpbc_gt_multi_exp(x.data(), nullptr, 0, seg, 1, &z));
    return z;
}

// bn254.Pair: product of pairings, one final exponentiation.  gnark's error: "invalid inputs sizes".
inline GT Pair(const std::vector<G1Affine> &P, const std::vector<G2Affine> &Q) {
    if (P.empty() || P.size() != Q.size()) throw std::invalid_argument("invalid inputs sizes");
    uint64_t seg[2] = {0, P.size()};
    GT out;
    check(gpbc_multi_pair(P.data(), Q.data(), seg, 1, &out));
    return out;
}
inline bool PairingCheck(const std::vector<G1Affine> &P, const std::vector<G2Affine> &Q) {
    if (P.empty() || P.size() != Q.size()) throw std::invalid_argument("invalid inputs sizes");
    uint64_t seg[2] = {0, P.size()};
    uint8_t ok = 0;
    check(gpbc_pairing_check(P.data(), Q.data(), seg, 1, &ok));
    return ok == 1;
}
// bn254.HashToG1(msg, dst) / HashToG2(msg, dst) (hash/hash_to.go:113-119,169-175,204-210,271-277; the BLS scheme hashes every
// message: signature/bls01_signature/bls_signature.go:56-63), hashing included; gnark errors on a DST longer than 255 bytes
inline std::vector<G1Affine> HashToG1Batch(const std::vector<std::string> &msgs, const std::string &dst) {
    if (dst.size() > 255) throw std::invalid_argument("invalid domain size (>255 bytes)");
    std::vector<G1Affine> out(msgs.size());
    std::string data;
    std::vector<uint64_t> off(msgs.size() + 1, 0);
    for (size_t i = 0; i < msgs.size(); i++) { data += msgs[i]; off[i + 1] = data.size(); }
    if (data.empty()) data.push_back('\0');
    check(gpbc_hash_to_g1(data.data(), off.data(), msgs.size(), dst.data(), dst.size(), out.data()));
    return out;
}
inline std::vector<G2Affine> HashToG2Batch(const std::vector<std::string> &msgs, const std::string &dst) {
    if (dst.size() > 255) throw std::invalid_argument("invalid domain size (>255 bytes)");
    std::vector<G2Affine> out(msgs.size());
    std::string data;
    std::vector<uint64_t> off(msgs.size() + 1, 0);
    for (size_t i = 0; i < msgs.size(); i++) { data += msgs[i]; off[i + 1] = data.size(); }
    if (data.empty()) data.push_back('\0');
    check(gpbc_hash_to_g2(data.data(), off.data(), msgs.size(), dst.data(), dst.size(), out.data()));
    return out;
}
inline G1Affine HashToG1(const std::string &msg, const std::string &dst) { return HashToG1Batch({msg}, dst)[0]; }
inline G2Affine HashToG2(const std::string &msg, const std::string &dst) { return HashToG2Batch({msg}, dst)[0]; }
// h(u, v, w) of Gentry06 (ibe/gentry06_ibe/gentry06_ibe.go:319-343) for n items, and fr.SetBytes(SHA-256(msg)) per message (gpbc_bn254_hash.h)
inline std::vector<Scalar> HashG1GTGTToFr(const std::vector<G1Affine> &u, const std::vector<GT> &v, const std::vector<GT> &w) {
    if (u.size() != v.size() || u.size() != w.size()) throw std::invalid_argument("invalid inputs sizes");
    std::vector<Scalar> out(u.size());
    check(gpbc_hash_g1_gt_gt_to_fr(u.data(), v.data(), w.data(), u.size(), out.data()));
    return out;
}
inline std::vector<Scalar> Sha256ToFrBatch(const std::vector<std::string> &msgs) {
    std::vector<Scalar> out(msgs.size());
    std::string data;
    std::vector<uint64_t> off(msgs.size() + 1, 0);
    for (size_t i = 0; i < msgs.size(); i++) { data += msgs[i]; off[i + 1] = data.size(); }
    if (data.empty()) data.push_back('\0');
    check(gpbc_sha256_batch(data.data(), off.data(), msgs.size(), 1, out.data()));
    return out;
}
// batched forms the engine adds
inline std::vector<GT> PairBatch(const std::vector<G1Affine> &P, const std::vector<G2Affine> &Q) {
    if (P.empty() || P.size() != Q.size()) throw std::invalid_argument("invalid inputs sizes");
    std::vector<GT> out(P.size());
    check(gpbc_pair_batch(P.data(), Q.data(), P.size(), out.data()));
    return out;
}
inline std::vector<G1Affine> G1ScalarMultiplicationBatch(const std::vector<G1Affine> &bases, const std::vector<Scalar> &s) {
    std::vector<G1Affine> out(s.size());
    check(gpbc_g1_scalar_mul_batch(bases.data(), bases.size(), s.data(), s.size(), out.data()));
    return out;
}
inline std::vector<G2Affine> G2ScalarMultiplicationBatch(const std::vector<G2Affine> &bases, const std::vector<Scalar> &s) {
    std::vector<G2Affine> out(s.size());
    check(gpbc_g2_scalar_mul_batch(bases.data(), bases.size(), s.data(), s.size(), out.data()));
    return out;
}
// out[i] = a[i] + b[i] / a[i] - b[i] / 2 a[i]: batched G1Affine.Add / Sub / Double (and G2); b holds a.size() points or one point
// for all (a public key added to every [H(m_i)]g2).  A single Add or Neg is cheaper in place on the host (G1Affine::Neg above).
namespace detail {
template <class P, class Fn> inline std::vector<P> group_op(const std::vector<P> &a, const std::vector<P> &b, Fn fn) {
    if (b.size() != 1 && b.size() != a.size()) throw std::invalid_argument("need one b or one b per a");
    std::vector<P> out(a.size());
    check(fn(a.data(), b.data(), b.size(), a.size(), out.data()));
    return out;
}
}  // namespace detail
inline std::vector<G1Affine> G1AddBatch(const std::vector<G1Affine> &a, const std::vector<G1Affine> &b) { return detail::group_op(a, b, gpbc_g1_add_batch); }
inline std::vector<G1Affine> G1SubBatch(const std::vector<G1Affine> &a, const std::vector<G1Affine> &b) { return detail::group_op(a, b, gpbc_g1_sub_batch); }
inline std::vector<G1Affine> G1DoubleBatch(const std::vector<G1Affine> &a) {
    std::vector<G1Affine> out(a.size());
    check(gpbc_g1_double_batch(a.data(), a.size(), out.data()));
    return out;
}
inline std::vector<G2Affine> G2AddBatch(const std::vector<G2Affine> &a, const std::vector<G2Affine> &b) { return detail::group_op(a, b, gpbc_g2_add_batch); }
inline std::vector<G2Affine> G2SubBatch(const std::vector<G2Affine> &a, const std::vector<G2Affine> &b) { return detail::group_op(a, b, gpbc_g2_sub_batch); }
inline std::vector<G2Affine> G2DoubleBatch(const std::vector<G2Affine> &a) {
    std::vector<G2Affine> out(a.size());
    check(gpbc_g2_double_batch(a.data(), a.size(), out.data()));
    return out;
}
// fr.Element arithmetic on scalars, n at a time (gpbc_bn254.h "scalar field"): out[i] = a[i] + b[i] / - / * (b of one scalar: the same b
// for every a), -a[i], 1 / a[i] (0 for 0, gnark's Inverse).  Inputs act as their residue modulo r, outputs are canonical.
namespace detail {
template <class Fn> inline std::vector<Scalar> fr_binary(const std::vector<Scalar> &a, const std::vector<Scalar> &b, Fn fn) {
    if (b.size() != 1 && b.size() != a.size()) throw std::invalid_argument("need one b or one b per a");
    std::vector<Scalar> out(a.size());
    check(fn(a.data(), b.data(), b.size(), a.size(), out.data()));
    return out;
}
template <class Fn> inline std::vector<Scalar> fr_unary(const std::vector<Scalar> &a, Fn fn) {
    std::vector<Scalar> out(a.size());
    check(fn(a.data(), a.size(), out.data()));
    return out;
}
}  // namespace detail
inline std::vector<Scalar> FrAddBatch(const std::vector<Scalar> &a, const std::vector<Scalar> &b) { return detail::fr_binary(a, b, gpbc_fr_add_batch); }
inline std::vector<Scalar> FrSubBatch(const std::vector<Scalar> &a, const std::vector<Scalar> &b) { return detail::fr_binary(a, b, gpbc_fr_sub_batch); }
inline std::vector<Scalar> FrMulBatch(const std::vector<Scalar> &a, const std::vector<Scalar> &b) { return detail::fr_binary(a, b, gpbc_fr_mul_batch); }
inline std::vector<Scalar> FrNegBatch(const std::vector<Scalar> &a) { return detail::fr_unary(a, gpbc_fr_neg_batch); }
inline std::vector<Scalar> FrInverseBatch(const std::vector<Scalar> &a) { return detail::fr_unary(a, gpbc_fr_inverse_batch); }
// fr.Element's in-memory words (Montgomery, R = 2^256) <-> Scalar
inline std::vector<Scalar> FrFromMontBatch(const std::vector<Scalar> &a) { return detail::fr_unary(a, gpbc_fr_from_mont_batch); }
inline std::vector<Scalar> FrToMontBatch(const std::vector<Scalar> &a) { return detail::fr_unary(a, gpbc_fr_to_mont_batch); }
// k polynomials prod_i (X - roots[j*B + i]) of B roots each: k x (B + 1) coefficients, constant term first (computePolynomialCoeffs)
inline std::vector<Scalar> FrPolyFromRoots(const std::vector<Scalar> &roots, size_t B) {
    if (B < 1 || roots.size() % B) throw std::invalid_argument("need B roots per polynomial");
    std::vector<Scalar> out(roots.size() / B * (B + 1));
    check(gpbc_fr_poly_from_roots(roots.data(), B, roots.size() / B, out.data()));
    return out;
}
// row j*B + i: the B coefficients of coeffs[j](X) / (X - points[j*B + i]) and stride - B zeros; ok[j*B + i] = 0 (and a zero row) where the
// division leaves a remainder.  A row is one row of G1FixedBase::Msm over stride bases.
inline std::vector<Scalar> FrPolyQuotients(const std::vector<Scalar> &coeffs, const std::vector<Scalar> &points, size_t B, size_t stride, std::vector<uint8_t> &ok) {
    if (B < 1 || stride < B || points.size() % B || coeffs.size() != points.size() / B * (B + 1)) throw std::invalid_argument("invalid inputs sizes");
    std::vector<Scalar> out(points.size() * stride);
    ok.assign(points.size(), 0);
    check(gpbc_fr_poly_quotients(coeffs.data(), points.data(), B, points.size() / B, stride, out.data(), ok.data()));
    return out;
}
// Lagrange basis for k rows (utils.ComputeLagrangeBasis with a node set per item): out[j*m + t] = prod over the elements s of set row j with
// s != node t of row j (mod r) of (x[j] - s) / (node - s).  set: one row of B or k rows; nodes: empty = the set's own elements, else one
// row of m or k rows; x: empty = evaluate at 0, else one scalar or k.  k is the largest of the three row counts.
inline std::vector<Scalar> FrLagrangeBasis(const std::vector<Scalar> &set, size_t B, const std::vector<Scalar> &nodes = {}, size_t m = 0, const std::vector<Scalar> &x = {}) {
    if (B < 1 || set.empty() || set.size() % B) throw std::invalid_argument("need B set elements per row");
    if (nodes.empty()) m = B;
    else if (m < 1 || nodes.size() % m) throw std::invalid_argument("need m nodes per row");
    const size_t ns = set.size() / B, nn = nodes.empty() ? ns : nodes.size() / m, nx = x.size(), k = std::max(ns, std::max(nn, nx));
    if ((ns != 1 && ns != k) || (nn != 1 && nn != k) || (nx > 1 && nx != k)) throw std::invalid_argument("need one row or one row per output row");
    std::vector<Scalar> out(k * m);
    check(gpbc_fr_lagrange_basis(set.data(), ns, B, nodes.empty() ? nullptr : nodes.data(), nn, m, x.empty() ? nullptr : x.data(), nx, k, out.data()));
    return out;
}
// Polynomial evaluation for k rows (utils.ComputePolynomialValue): out[j*m + t] = sum_i coeffs[j*d + i] points[j*m + t]^i, coefficients
// lowest degree first.  coeffs: one row of d or k rows; points: one row of m or k rows; k is the larger row count.
inline std::vector<Scalar> FrPolyEval(const std::vector<Scalar> &coeffs, size_t d, const std::vector<Scalar> &points, size_t m) {
    if (d < 1 || coeffs.empty() || coeffs.size() % d) throw std::invalid_argument("need d coefficients per row");
    if (m < 1 || points.empty() || points.size() % m) throw std::invalid_argument("need m points per row");
    const size_t nc = coeffs.size() / d, np = points.size() / m, k = std::max(nc, np);
    if ((nc != 1 && nc != k) || (np != 1 && np != k)) throw std::invalid_argument("need one row or one row per output row");
    std::vector<Scalar> out(k * m);
    check(gpbc_fr_poly_eval(coeffs.data(), nc, d, points.data(), np, m, k, out.data()));
    return out;
}
// A threshold tree uploaded once (AccessTreeNode.ShareSecret for k secrets per call): nodes in depth-first preorder, node i =
// (parent, threshold), parent GPBC_SHARE_ROOT for node 0, threshold 0 = a leaf.  Share returns k x Leaves() scalars, item-major, leaf order.
class ShareTree {
public:
    explicit ShareTree(const std::vector<gpbc_share_node> &nodes) { check(gpbc_share_tree_create(nodes.data(), nodes.size(), &h_)); }
    ShareTree(const ShareTree &) = delete;
    ShareTree &operator=(const ShareTree &) = delete;
    ~ShareTree() { gpbc_share_tree_destroy(h_); }
    size_t Leaves() const { return gpbc_share_tree_leaves(h_); }
    size_t Coeffs() const { return gpbc_share_tree_coeffs(h_); }
    std::vector<Scalar> Share(const std::vector<Scalar> &secrets, const std::vector<Scalar> &coeffs) const {
        if (coeffs.size() != secrets.size() * Coeffs()) throw std::invalid_argument("need Coeffs() coefficients per secret");
        std::vector<Scalar> out(secrets.size() * Leaves());
        check(gpbc_fr_share_tree(h_, secrets.data(), coeffs.empty() ? nullptr : coeffs.data(), secrets.size(), out.data()));
        return out;
    }
private:
    gpbc_share_tree *h_ = nullptr;
};
// LSSS reconstruction weights for k systems (FindLinearCombinationWeight with a matrix per item): matrix holds one rows x cols matrix or
// k of them, held k x rows bytes (non-zero: the key holds the row's attribute).  Returns k x rows weights (0 where a row is not used)
// and fills ok with k bytes (0: the held rows do not span (1, 0, ..., 0); that row of weights is then all zero).
inline std::vector<Scalar> FrLsssWeights(const std::vector<Scalar> &matrix, size_t rows, size_t cols, const std::vector<uint8_t> &held, std::vector<uint8_t> &ok) {
    if (rows < 1 || cols < 1 || matrix.empty() || matrix.size() % (rows * cols) || held.size() % rows) throw std::invalid_argument("need rows x cols scalars per matrix, rows bytes per mask");
    const size_t nm = matrix.size() / (rows * cols), k = held.size() / rows;
    if (nm != 1 && nm != k) throw std::invalid_argument("need one matrix or one per mask");
    std::vector<Scalar> w(k * rows);
    ok.assign(k, 0);
    check(gpbc_fr_lsss_weights(matrix.data(), nm, rows, cols, held.data(), k, w.data(), ok.data()));
    return w;
}
// k products against ONE list of G2 points (a decryption key against k ciphertexts): out[j] = Pair(P[j*m .. (j+1)*m), Q);
// the Miller lines of Q are computed once (gnark: PrecomputeLines / MillerLoopFixedQ)
inline std::vector<GT> PairFixedQ(const std::vector<G1Affine> &P, const std::vector<G2Affine> &Q) {
    if (Q.empty() || P.empty() || P.size() % Q.size()) throw std::invalid_argument("invalid inputs sizes");
    std::vector<GT> out(P.size() / Q.size());
    check(gpbc_multi_pair_fixed_q(P.data(), Q.data(), Q.size(), out.size(), out.data()));
    return out;
}
// Fixed-base window tables in HBM: ScalarMultiplicationBase-style batches and sums  sum_j [s_j] base_j  over fixed bases
class G1FixedBase {
public:
    explicit G1FixedBase(const std::vector<G1Affine> &bases) : n_(bases.size()) { check(gpbc_g1_fixed_base_create(bases.data(), bases.size(), &h_)); }
    ~G1FixedBase() { gpbc_fixed_base_destroy(h_); }
    G1FixedBase(const G1FixedBase &) = delete;
    G1FixedBase &operator=(const G1FixedBase &) = delete;
    // scalars: n_msm rows of NBases() scalars; one point per row
    std::vector<G1Affine> Msm(const std::vector<Scalar> &scalars) const {
        if (scalars.size() % n_) throw std::invalid_argument("need one scalar per base and sum");
        std::vector<G1Affine> out(scalars.size() / n_);
        check(gpbc_fixed_base_msm(h_, scalars.data(), out.size(), out.data()));
        return out;
    }
    // out[i] = sum_{t < terms} [scalars[i * terms + t]] base[index[(i % rows) * terms + t]] (include/gpbc_bn254_indexed.h): index holds
    // rows x terms entries, rows == the number of outputs or fewer (periodic); GPBC_INDEX_NONE = no term; ok[i] = 0 and an all-zero point
    // where an index names no base
    std::vector<G1Affine> Indexed(const std::vector<uint32_t> &index, size_t terms, const std::vector<Scalar> &scalars, std::vector<uint8_t> &ok) const {
        if (terms < 1 || index.empty() || index.size() % terms || scalars.size() % terms) throw std::invalid_argument("need whole rows of `terms` indices and scalars");
        std::vector<G1Affine> out(scalars.size() / terms);
        ok.assign(out.size(), 0);
        check(gpbc_fixed_base_indexed(h_, index.data(), index.size() / terms, terms, scalars.data(), out.size(), out.data(), ok.data()));
        return out;
    }
    size_t NBases() const { return n_; }
private:
    gpbc_fixed_base *h_ = nullptr;
    size_t n_;
};
// LSSS shares lambda_x = M_x . v for k vectors (LewkoWatersLsssMatrix.ComputeVector per item): matrix holds one rows x cols matrix or k of
// them, vectors k x cols scalars.  Returns k x rows canonical scalars.
inline std::vector<Scalar> FrLsssShares(const std::vector<Scalar> &matrix, size_t rows, size_t cols, const std::vector<Scalar> &vectors) {
    if (rows < 1 || cols < 1 || matrix.empty() || matrix.size() % (rows * cols) || vectors.size() % cols) throw std::invalid_argument("need rows x cols scalars per matrix, cols per vector");
    const size_t nm = matrix.size() / (rows * cols), k = vectors.size() / cols;
    if (k && nm != 1 && nm != k) throw std::invalid_argument("need one matrix or one per vector");
    std::vector<Scalar> out(k * rows);
    check(gpbc_fr_lsss_shares(matrix.data(), nm, rows, cols, vectors.data(), k, out.data()));
    return out;
}
// FindCommonAttributes(set, list, d) for k lists of `a` scalars (include/gpbc_bn254_select.h): sets holds one set of m scalars or k of them.
// Per item and slot s < d: the s-th kept element's position in the set and in the list, and its canonical value; ok[j] = 0 and zero rows
// where fewer than d are common.
struct CommonAttributes {
    std::vector<uint32_t> set_pos, list_pos;      // k x d
    std::vector<Scalar> common;                   // k x d
    std::vector<uint8_t> ok;                      // k
};
inline CommonAttributes FrFindCommon(const std::vector<Scalar> &sets, size_t m, const std::vector<Scalar> &lists, size_t a, size_t d) {
    if (m < 1 || a < 1 || d < 1 || sets.empty() || sets.size() % m || lists.size() % a) throw std::invalid_argument("need m scalars per set, a per list");
    const size_t n_sets = sets.size() / m, k = lists.size() / a;
    if (k && n_sets != 1 && n_sets != k) throw std::invalid_argument("need one set or one per list");
    CommonAttributes out{std::vector<uint32_t>(k * d), std::vector<uint32_t>(k * d), std::vector<Scalar>(k * d), std::vector<uint8_t>(k)};
    check(gpbc_fr_find_common(sets.data(), n_sets, m, lists.data(), a, d, k, out.set_pos.data(), out.list_pos.data(), out.common.data(), out.ok.data()));
    return out;
}
static_assert(sizeof(Scalar) == GPBC_SCALAR_BYTES, "scalar layout");

}  // namespace bn254
#endif
