// Host build of the DEVICE arithmetic (csrc/fe29.hip.hpp, tower29.hip.hpp, curve29.hip.hpp, pairing29.hip.hpp, group29.hip.hpp ...) with -DGPBC_BOUNDS:
// every field element carries data-independent magnitude bounds and every product asserts that its int64 column
// accumulators cannot overflow (abort() on violation).  This is a verification harness for tests/ only — it is
// never loaded by the product path (which has no CPU fallback).
//
// build: g++ -O2 -std=c++17 -DGPBC_BOUNDS -shared -fPIC -o tools/libgpbc_bounds.so tools/bounds_check.cpp
#ifndef GPBC_BOUNDS
#define GPBC_BOUNDS
#endif
#include <algorithm>
#include <cstring>
#include <tuple>
#include "../gopairingbasedcryptography_amd/csrc/curve29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/pairing29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/pairing29_pair.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/wide29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/wire29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/h2c29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/msm29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/group29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/fr29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/gtmexp29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/gmsm29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/subset29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/transcript29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/share29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/recon29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/lsss29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/select29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/formula29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/fbindex29.hip.hpp"
#include "../gopairingbasedcryptography_amd/csrc/chacha29.hip.hpp"
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

using namespace gpbc;

// Host stand-in for the DPP lane swap: the two lanes of a pair run as two threads; swap() is a rendezvous.
struct PairRendezvous {
    std::mutex mu; std::condition_variable cv;
    const void *slot[2] = {nullptr, nullptr}; int arrived = 0, left = 0; long gen = 0;
    template <class T> T exchange(int me, const T &v) {
        std::unique_lock<std::mutex> lk(mu);
        while (left != 0) cv.wait(lk);                 // previous exchange fully drained
        slot[me] = &v;
        long g = gen;
        if (++arrived == 2) { gen++; left = 2; cv.notify_all(); }
        else while (gen == g) cv.wait(lk);
        T out = *static_cast<const T *>(slot[1 - me]);
        if (--left == 0) { arrived = 0; cv.notify_all(); }
        else while (left != 0) cv.wait(lk);            // keep my value alive until the partner has copied it
        return out;
    }
};
struct PairHost {
    bool odd; PairRendezvous *rv;
    Fe swap(const Fe &a) const { return rv->exchange<Fe>(odd, a); }
    F2 swap(const F2 &a) const { return rv->exchange<F2>(odd, a); }
    F6 swap(const F6 &a) const { return rv->exchange<F6>(odd, a); }
    Fe sgn(const Fe &a) const { return odd ? a : fe_neg(a); }                       // device: one multiplication by the lane's +-1
    Fe add_swap(const Fe &a, const Fe &b) const { return fe_add(a, swap(b)); }       // device: v_add_u32_dpp
    static bool all(bool c) { return c; }                                            // device: the whole wavefront must agree
};
static std::mutex g_stats_mu;
static BoundStats g_stats_total;
static void stats_flush() { std::lock_guard<std::mutex> lk(g_stats_mu); bound_stats_merge(g_stats_total, bound_stats()); }

template <class F, class LoadA, class StoreA> static void smul_batch(const uint8_t *B, const uint8_t *K, size_t n, uint8_t *out, size_t pt, LoadA ld, StoreA st) {
    constexpr int KK = 4;                                  // same grouping as the kernels: one shared inversion per 4 points
    size_t T = (n + KK - 1) / KK;
    for (size_t t = 0; t < T; t++) {
        JacP<F> res[KK];
        for (int j = 0; j < KK; j++) {
            size_t i = t + (size_t)j * T;
            if (i >= n) { jac_set_inf(res[j]); continue; }
            uint32_t k[8]; memcpy(k, K + 32 * i, 32);
            alignas(16) int32_t tab[glv_table_dwords<F>()];
            scalar_mul29_best(res[j], ld(B + pt * i), k, tab);
        }
        AffP<F> aff[KK];
        jac_to_affine_batch<F, KK>(aff, res);
        for (int j = 0; j < KK; j++) { size_t i = t + (size_t)j * T; if (i < n) st(out + pt * i, aff[j]); }
    }
}

// Bucket MSM exactly as csrc/gpbc_msm.hip runs it — the same per-lane pieces of msm29.hip.hpp in the same order (bucket sums by
// mixed additions, group reduction with the small multiplication, fan-in sums, Horner over the windows) — with the points kept as
// objects so that their tracked intervals flow from step to step.  out = sum_i [K_i] B_i (affine, gnark layout).
template <class F, class LoadA, class StoreA> static void msm_host(const uint8_t *B, const uint8_t *K, size_t n, int c, uint8_t *out, size_t pt, LoadA ld, StoreA st) {
    const int W = (256 + c - 1) / c;
    const size_t nb = (size_t)1 << c;
    std::vector<std::vector<size_t>> members((size_t)W * nb);
    for (size_t i = 0; i < n; i++) {
        if (bytes_all_zero(B + pt * i, (int)(pt / 4))) continue;
        uint32_t k[8]; memcpy(k, K + 32 * i, 32);
        for (int w = 0; w < W; w++) { uint32_t d = msm_digit(k, w, c); if (d) members[(size_t)w * nb + d].push_back(i); }
    }
    std::vector<JacP<F>> buckets((size_t)W * nb);
    for (size_t key = 0; key < buckets.size(); key++) {
        const auto &m = members[key];
        msm_bucket_sum(buckets[key], 0, m.size(), [&](size_t j) { return ld(B + pt * m[j]); });
    }
    const size_t gpw = nb >= (size_t)MSM_GROUP ? nb / MSM_GROUP : 1, gsz = nb >= (size_t)MSM_GROUP ? MSM_GROUP : nb;
    std::vector<JacP<F>> wsum(W);
    for (int w = 0; w < W; w++) {
        JacP<F> acc, s; jac_set_inf(acc);
        for (size_t g = 0; g < gpw; g++) {
            JacP<F> r;
            uint32_t lo = (uint32_t)(g * gsz), hi = lo + (uint32_t)gsz - 1;
            msm_group_reduce(r, lo ? lo : 1u, hi, [&](uint32_t d) { return buckets[(size_t)w * nb + d]; });
            jac_add(s, acc, r); acc = s;
        }
        wsum[w] = acc;
    }
    JacP<F> acc = wsum[W - 1];
    for (int w = W - 2; w >= 0; w--) msm_horner_step(acc, wsum[w], c);
    AffP<F> a; jac_to_affine(a, acc);
    st(out, a);
}
// host memory policy of the latency ("wide") form, csrc/wide29.hip.hpp: the slots are interval-carrying values, the lanes of a
// phase run one after the other and their stores land when the phase ends (what the barrier does on the device)
struct WideHost {
    static constexpr bool LIMB_PARALLEL = false;          // the device spreads some linear phases over one limb per lane; the host runs their Fe-level form
    std::vector<F2> s = std::vector<F2>(W_SLOTS, f2_zero());
    std::vector<std::pair<int, F2>> pending;
    std::vector<std::tuple<int, int, Fe>> pending_half;
    F2 ld(int i) const { return s[i]; }
    Fe ldh(int i, int h) const { return h ? s[i].a1 : s[i].a0; }
    void st(int i, const F2 &v) { pending.emplace_back(i, v); }
    void sth(int i, int h, const Fe &v) { pending_half.emplace_back(i, h, v); }
    int waves() const { return 2; }                        // the form with the helper wave (half products in wide_mul); the one-wave form multiplies whole F2 products: f2_mul, covered by the throughput kernels' runs
    template <class B> void run2(int n, B &&body) { run(n, body); }
    void sync_waves() const {}
    template <class B> void limbs(int n_comp, B &&body) { LimbOpsFe<WideHost> o{*this}; run(n_comp, [&](int c) { body(o, c); }); }
    template <class B> void run(int n, B &&body) {
        for (int l = 0; l < n; l++) body(l);
        for (auto &p : pending) s[p.first] = p.second;
        for (auto &p : pending_half) (std::get<1>(p) ? s[std::get<0>(p)].a1 : s[std::get<0>(p)].a0) = std::get<2>(p);
        pending.clear(); pending_half.clear();
    }
};
// elementwise group law exactly as k_g1_add .. k_g2_dbl (csrc/gpbc_group.hip) run it: the same lane function of group29.hip.hpp with
// the same grouping (lane t owns elements t, t + T, ... with T = ceil(n / k)); op 0 ADD, 1 SUB, 2 DBL; nb = 1 broadcasts B[0].
// k = 0 takes the kernels' K (GROUP_K_G1 / GROUP_K_G2).  No cross-lane step: every lane runs on its own, one after the other.
template <class F, int K> static void group_host(int op, const uint8_t *A, const uint8_t *B, size_t nb, size_t n, uint8_t *out) {
    const size_t T = (n + K - 1) / K, step = nb == n && op != GROUP_DBL ? GroupPt<F>::BYTES : 0;
    for (size_t t = 0; t < T; t++) {
        if (op == GROUP_ADD) group_op_lane<F, K, GROUP_ADD>(A, B, step, out, n, t, T);
        else if (op == GROUP_SUB) group_op_lane<F, K, GROUP_SUB>(A, B, step, out, n, t, T);
        else group_op_lane<F, K, GROUP_DBL>(A, A, 0, out, n, t, T);
    }
}
// the inversion kernel's lanes (hc_fr_op), k elements each
template <int K> static void fr_inverse_host(const uint8_t *A, size_t n, uint8_t *out) {
    const size_t T = (n + K - 1) / K;
    for (size_t t = 0; t < T; t++) fr_inverse_lane<K>(A, out, n, t, T);
}
// k_fr_lagrange_basis: the sets made canonical once (what the workgroup stages), then fr_lagrange_lane for every lane of every row
// with the kernel's grouping (g = 0: FR_LAGRANGE_G outputs per lane at gi, gi + gpr, ...).  nodes null = the set's own elements,
// x null = 0; n_set_rows / n_node_rows in {1, k}, nx in {0, 1, k}.
template <int G> static void fr_lagrange_host(const uint8_t *set, size_t n_set_rows, size_t B, const uint8_t *nodes, size_t n_node_rows, size_t m, const uint8_t *x, size_t nx,
                                              size_t k, uint8_t *out) {
    const uint32_t gpr = (uint32_t)((m + G - 1) / G);
    std::vector<Fr> ss(B);
    for (size_t j = 0; j < k; j++) {
        if (j == 0 || n_set_rows != 1)
            for (size_t u = 0; u < B; u++) ss[u] = fr_lagrange_in(set + ((n_set_rows == 1 ? 0 : j) * B + u) * 32);
        const Fr xc = x ? fr_lagrange_in(x + (nx == 1 ? 0 : j) * 32) : fr_zero();
        const uint8_t *nd = nodes ? nodes + (n_node_rows == 1 ? 0 : j) * m * 32 : nullptr;
        for (uint32_t gi = 0; gi < gpr; gi++)
            fr_lagrange_lane<G>([&](uint32_t u) { return ss[u]; }, (uint32_t)B, nd, xc, (uint32_t)m, gi, gpr, out + j * m * 32);
    }
}
// k_fr_lsss_weights, one workgroup: the staging, then per unknown the ballot of fr_lsss_nonzero over the 64 lanes, fr_lsss_step for
// every lane, (the barrier,) fr_lsss_clear; the last ballot and fr_lsss_finish — the kernel's sequence with the lanes in turn.
template <class Get, class Put> static void fr_lsss_block(const LsssGeom &g, uint32_t block, size_t k, const uint8_t *matrix, size_t mat_step, const uint8_t *held, const Get &get,
                                                          const Put &put, uint8_t *w_out, uint8_t *ok_out, uint32_t *active) {
    for (uint32_t lane = 0; lane < FR_LSSS_WAVE; lane++) fr_lsss_stage(g, block, lane, k, matrix, mat_step, held, put);
    LsssLane l[FR_LSSS_WAVE];
    LsssState st[FR_LSSS_WAVE];
    for (uint32_t lane = 0; lane < FR_LSSS_WAVE; lane++) {
        l[lane] = fr_lsss_map(g, block, lane, k);
        st[lane] = fr_lsss_begin(g);
        if (active && l[lane].active && l[lane].li < g.rows) ++*active;
    }
    for (uint32_t c = 0; c <= g.rows; c++) {
        uint64_t nz = 0;
        for (uint32_t lane = 0; lane < FR_LSSS_WAVE; lane++) nz |= (uint64_t)fr_lsss_nonzero(g, l[lane], c, get) << lane;
        if (c == g.rows) {
            for (uint32_t lane = 0; lane < FR_LSSS_WAVE; lane++) fr_lsss_finish(g, l[lane], nz, st[lane], get, w_out, ok_out);
            break;
        }
        for (uint32_t lane = 0; lane < FR_LSSS_WAVE; lane++) fr_lsss_step(g, l[lane], c, nz, st[lane], get, put);
        for (uint32_t lane = 0; lane < FR_LSSS_WAVE; lane++) fr_lsss_clear(g, l[lane], c, st[lane], put);
    }
}
// segmented multi-scalar multiplication exactly as gpbc_g1/g2_multi_scalar_mul_dev (csrc/gpbc_gmsm.hip) run it: the plan and the level
// walk of csrc/segred29.hip.hpp with GMSM_SHAPE (segred_piece per piece, the function the kernel calls; the value buffers sized by
// segred_plan), the same lane functions (gmsm_lane; gmsm_sum_lane for K = null and for the folds), one piece per lane, the lanes one
// after the other.
template <class F, class LoadA, class StoreA> static void gmsm_host(const uint8_t *B, const uint8_t *K, size_t nk, const uint64_t *seg_off, size_t n, size_t n_seg, uint8_t *out,
                                                                     size_t pt, LoadA ld, StoreA st) {
    const SegRedPlan plan = segred_plan(GMSM_SHAPE, pt, sizeof(int32_t) * (size_t)gmsm_lane_dwords<F>(), n, n_seg, K != nullptr);
    std::vector<uint8_t> v0(plan.val_bytes[0]), v1(plan.val_bytes[1]);
    uint8_t *const val[2] = {v0.data(), v1.data()};
    std::vector<int32_t> block(gmsm_lane_dwords<F>() + 32);
    int32_t *ws = block.data();
    while ((uintptr_t)ws & 127) ws++;                      // the lane's block: 128-byte aligned like the device's
    segred_walk(GMSM_SHAPE, segred_args(B, K, nk, seg_off, n, n_seg), val, out, [&](SegRedArgs g, size_t pieces) {
        g.n_pieces = pieces;
        for (size_t lane = 0; lane < pieces; lane++) {
            size_t lo, a, b, P;
            segred_piece(g, lane, lo, a, b, P);
            const size_t k0 = g.k_shared ? lo : 0;
            auto base = [&](size_t i) { return ld(g.x + (a + i) * pt); };
            JacP<F> r = g.k ? gmsm_lane<F>(b - a, base, [&](size_t i, uint32_t *k) { memcpy(k, g.k + 32 * (a + i - k0), 32); }, ws) : gmsm_sum_lane<F>(b - a, base);
            AffP<F> o;
            jac_to_affine(o, r);
            st(g.out + P * pt, o);
        }
        return 0;
    });
}
// bit-selected sums exactly as gpbc_subset_sum_dev (csrc/gpbc_subset.hip) runs them: subset_entry per table row, subset_shape's chunks,
// subset_lane per (item, chunk), the chunk-major partial sums folded as the strided point-sum kernel folds them.  Only the rows the
// masks reach are built (a row depends on nothing but its own (w, v)), plus the row a window past W reads.  n_shape != 0: the chunks of
// a call of n_shape items (so that a few items walk the one long chain of a call that fills the chip).
template <class F, class LoadA, class StoreA> static void subset_host(const uint8_t *B, size_t nbits, const uint8_t *O, const uint8_t *masks, size_t n, size_t n_shape, uint8_t *out,
                                                                       size_t pt, LoadA ld, StoreA st) {
    const size_t W = subset_windows(nbits), entries = subset_entries(nbits);
    constexpr size_t ED = (size_t)TabLayout<F>::ENTRY_DWORDS;
    std::vector<int32_t> mem(entries * ED + 32);
    int32_t *table = mem.data();
    while ((uintptr_t)table & 127) table++;                // rows 128-byte aligned like the device's
    std::vector<uint8_t> flags(entries, 0), built(entries, 0);
    AffP<F> off;
    if (O) off = ld(O);
    auto build = [&](size_t e) {
        if (built[e]) return;
        AffP<F> a;
        subset_entry<F>(a, [&](size_t i) { return ld(B + i * pt); }, nbits, O ? &off : nullptr, e >> 8, (int)(e & 255));
        subset_entry_store<F>(table, flags.data(), e, a);
        built[e] = 1;
    };
    build((W - 1) * 256);
    for (size_t m = 0; m < n; m++)
        for (size_t w = 0; w < W; w++) build(w * 256 + masks[m * W + w]);
    size_t C, n_chunks;
    subset_shape(W, n_shape ? n_shape : n, C, n_chunks);
    std::vector<uint8_t> partial(n_chunks > 1 ? n_chunks * n * pt : 0);
    uint8_t *dst = n_chunks > 1 ? partial.data() : out;
    for (size_t t = 0; t < n * n_chunks; t++) {
        const size_t m = t % n, c = t / n;
        JacP<F> acc = subset_lane<F>(table, flags.data(), masks + m * W, W, c * C, C);
        AffP<F> a;
        jac_to_affine(a, acc);
        st(dst + t * pt, a);
    }
    if (n_chunks > 1)
        for (size_t t = 0; t < n; t++) {
            JacP<F> acc;
            jac_set_inf(acc);
            for (size_t i = t; i < n * n_chunks; i += n) jac_add_mixed(acc, acc, ld(dst + i * pt));
            AffP<F> r;
            jac_to_affine(r, acc);
            st(out + t * pt, r);
        }
}
extern "C" {

// out[m] = O + sum_{i : bit i of masks row m} B_i; O null = no offset; masks: n rows of ceil(nbits / 8) bytes
void hc_subset_sum(int is_g2, const uint8_t *B, size_t nbits, const uint8_t *O, const uint8_t *masks, size_t n, size_t n_shape, uint8_t *out) {
    if (is_g2)
        subset_host<F2>(B, nbits, O, masks, n, n_shape, out, 128, [](const uint8_t *p) { return AffP<F2>{f2_load(p), f2_load(p + 64), bytes_all_zero(p, 32)}; },
                        [](uint8_t *p, const AffP<F2> &r) { f2_store(p, r.x); f2_store(p + 64, r.y); });
    else
        subset_host<Fe>(B, nbits, O, masks, n, n_shape, out, 64, [](const uint8_t *p) { return AffP<Fe>{fe_load(p), fe_load(p + 32), bytes_all_zero(p, 16)}; },
                        [](uint8_t *p, const AffP<Fe> &r) { fe_store(p, r.x); fe_store(p + 32, r.y); });
    stats_flush();
}
// [max bits, windows per chunk at least, chunks of a call of n items over W windows, windows per chunk of it]
void hc_subset_shape(size_t W, size_t n, size_t *out4) {
    size_t C, n_chunks;
    subset_shape(W, n, C, n_chunks);
    out4[0] = SUBSET_MAX_BITS; out4[1] = SUBSET_CHUNK_MIN; out4[2] = n_chunks; out4[3] = C;
}
// out[s] = sum_{i in [seg_off[s], seg_off[s+1])} [K_i] B_i; nk = n, or one list of nk scalars for all segments; K null = plain sums
void hc_multi_scalar_mul(int is_g2, const uint8_t *B, const uint8_t *K, size_t nk, const uint64_t *seg_off, size_t n, size_t n_seg, uint8_t *out) {
    if (is_g2)
        gmsm_host<F2>(B, K, nk, seg_off, n, n_seg, out, 128, [](const uint8_t *p) { return AffP<F2>{f2_load(p), f2_load(p + 64), bytes_all_zero(p, 32)}; },
                      [](uint8_t *p, const AffP<F2> &r) { f2_store(p, r.x); f2_store(p + 64, r.y); });
    else
        gmsm_host<Fe>(B, K, nk, seg_off, n, n_seg, out, 64, [](const uint8_t *p) { return AffP<Fe>{fe_load(p), fe_load(p + 32), bytes_all_zero(p, 16)}; },
                      [](uint8_t *p, const AffP<Fe> &r) { fe_store(p, r.x); fe_store(p + 32, r.y); });
    stats_flush();
}
int hc_gmsm_group(int is_g2) { (void)is_g2; return GMSM_GROUP; }
// one pairing per "wavefront": Miller loop and final exponentiation of the latency form (k_miller_wide / k_final_exp_wide)
void hc_pair_wide(const uint8_t *P, const uint8_t *Q, size_t n, uint8_t *out, int do_final_exp) {
    for (size_t i = 0; i < n; i++) {
        const uint8_t *p = P + 64 * i, *q = Q + 128 * i;
        WideHost m;
        if (bytes_all_zero(p, 16) || bytes_all_zero(q, 32)) { m.s[0] = f2_one(); }
        else {
            G1A a{fe_load(p), fe_load(p + 32)};
            G2A b{f2_load(q), f2_load(q + 64)};
            std::vector<F2> ring;                          // the device passes the 88 lines through an LDS ring, wave to wave
            wide_miller_lines(m, a, b, [&](int) { m.run(3, [&](int t) { ring.push_back(m.ld(W_L0 + t)); }); });
            wide_miller_accumulate(m, wv(0), [&](int j) { m.run(3, [&](int t) { m.st(W_CL + t, ring[3 * j + t]); }); });
        }
        if (do_final_exp) wide_final_exp(m);
        for (int k = 0; k < 6; k++) f2_store(out + 384 * i + 64 * k, m.s[k]);
        stats_flush();
    }
}
// GT.Exp of the latency form (k_gt_exp_wide): x any Fp12 element, k a 256-bit plain exponent
void hc_gt_exp_wide(const uint8_t *x, const uint8_t *k, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; i++) {
        WideHost m;
        uint32_t kw[8];
        memcpy(kw, k + 32 * i, 32);
        for (int c = 0; c < 6; c++) m.s[wv(1) + c] = f2_load(x + 384 * i + 64 * c);
        wide_exp256(m, kw);
        for (int c = 0; c < 6; c++) f2_store(out + 384 * i + 64 * c, m.s[c]);
        stats_flush();
    }
}
void hc_pair(const uint8_t *P, const uint8_t *Q, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; i++) {
        const uint8_t *p = P + 64 * i, *q = Q + 128 * i;
        F12 f;
        if (bytes_all_zero(p, 16) || bytes_all_zero(q, 32)) f = f12_one();
        else {
            G1A a{fe_load(p), fe_load(p + 32)};
            G2A b{f2_load(q), f2_load(q + 64)};
            f = final_exp29(miller_loop29(a, b));
        }
        f12_store(out + 384 * i, f);
    }
}
void hc_miller(const uint8_t *P, const uint8_t *Q, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; i++) {
        G1A a{fe_load(P + 64 * i), fe_load(P + 64 * i + 32)};
        G2A b{f2_load(Q + 128 * i), f2_load(Q + 128 * i + 64)};
        f12_store(out + 384 * i, miller_loop29(a, b));
    }
}
void hc_final_exp(const uint8_t *F, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; i++) { F12 f; f12_load(f, F + 384 * i); f12_store(out + 384 * i, final_exp29(f)); }
}
void hc_g1_mul(const uint8_t *B, const uint8_t *K, size_t n, uint8_t *out) {
    smul_batch<Fe>(B, K, n, out, 64,
                   [](const uint8_t *p) { return AffP<Fe>{fe_load(p), fe_load(p + 32), bytes_all_zero(p, 16)}; },
                   [](uint8_t *p, const AffP<Fe> &r) { fe_store(p, r.x); fe_store(p + 32, r.y); });
}
void hc_g2_mul(const uint8_t *B, const uint8_t *K, size_t n, uint8_t *out) {
    smul_batch<F2>(B, K, n, out, 128,
                   [](const uint8_t *p) { return AffP<F2>{f2_load(p), f2_load(p + 64), bytes_all_zero(p, 32)}; },
                   [](uint8_t *p, const AffP<F2> &r) { f2_store(p, r.x); f2_store(p + 64, r.y); });
}
// GLV split of n 256-bit scalars: out rows = [k1 (5 x u32), k2 (5 x u32), neg1, neg2] as 12 u32
void hc_glv_split(const uint8_t *K, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        uint32_t k[8]; memcpy(k, K + 32 * i, 32);
        GlvSplit s; glv_split(s, k);
        memcpy(out + 12 * i, s.k1, 20); memcpy(out + 12 * i + 5, s.k2, 20);
        out[12 * i + 10] = s.neg1; out[12 * i + 11] = s.neg2;
    }
}
// G2 scalar multiplication by the two-dimensional GLV loop (the G2 kernels use the four-dimensional GLS loop; this keeps the
// GLV instantiation for F2 under test: the fixed-base table builder may use either)
void hc_g2_mul_glv(const uint8_t *B, const uint8_t *K, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; i++) {
        uint32_t k[8]; memcpy(k, K + 32 * i, 32);
        alignas(16) int32_t tab[glv_table_dwords<F2>()];
        AffP<F2> b{f2_load(B + 128 * i), f2_load(B + 128 * i + 64), bytes_all_zero(B + 128 * i, 32)}, r;
        JacP<F2> j;
        scalar_mul29_jac<F2>(j, b, k, tab);
        jac_to_affine(r, j);
        f2_store(out + 128 * i, r.x); f2_store(out + 128 * i + 64, r.y);
    }
}
// GLS split of n scalars: out rows = 4 x (3 magnitude words, sign) u32
void hc_gls_split(const uint8_t *K, size_t n, uint32_t *out) {
    for (size_t i = 0; i < n; i++) {
        uint32_t k[8]; memcpy(k, K + 32 * i, 32);
        GlsSplit s; gls_split(s, k);
        for (int c = 0; c < 4; c++) { memcpy(out + 16 * i + 4 * c, s.k[c], 12); out[16 * i + 4 * c + 3] = s.neg[c]; }
    }
}
void hc_fp_mul(const uint8_t *A, const uint8_t *B, size_t n, uint8_t *out) {
    // gnark-form a (= x R) and b (= y R), R = 2^256: internal product of the converted operands is x y R' -> stored as x y R
    for (size_t i = 0; i < n; i++) fe_store(out + 32 * i, fe_mul(fe_load(A + 32 * i), fe_load(B + 32 * i)));
}
// out = a^-1 by the safegcd inversion, out2 = by the Fermat power (gnark-form in and out: (xR)^-1 stored as x^-1 R)
void hc_fp_inv(const uint8_t *A, size_t n, uint8_t *out, uint8_t *out2) {
    for (size_t i = 0; i < n; i++) {
        Fe a = fe_load(A + 32 * i);
        fe_store(out + 32 * i, fe_inv(a));
        fe_store(out2 + 32 * i, fe_inv_fermat(a));
    }
}
// (a / p) by the divstep-based symbol: 1, -1, or 0 where it does not decide within its 960 steps (and for a = 0)
void hc_fp_legendre(const uint8_t *A, size_t n, int8_t *out) {
    for (size_t i = 0; i < n; i++) out[i] = (int8_t)fe_legendre(fe_load(A + 32 * i));
}
void hc_gt_mul(const uint8_t *A, const uint8_t *B, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; i++) { F12 a, b; f12_load(a, A + 384 * i); f12_load(b, B + 384 * i); f12_store(out + 384 * i, f12_mul(a, b)); }
}
// a / b as k_gt_binary computes it (norm-one divisors: conjugate instead of the Fp6 inversion)
void hc_gt_div(const uint8_t *A, const uint8_t *B, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; i++) {
        F12 a, b; f12_load(a, A + 384 * i); f12_load(b, B + 384 * i);
        f12_store(out + 384 * i, f12_mul(a, f12_inv_gt(b, [](bool c) { return c; })));
    }
}
void hc_gt_inv(const uint8_t *A, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; i++) { F12 a; f12_load(a, A + 384 * i); f12_store(out + 384 * i, f12_inv(a)); }
}
void hc_gt_sqr(const uint8_t *A, size_t n, uint8_t *out, int cyclo) {
    for (size_t i = 0; i < n; i++) { F12 a; f12_load(a, A + 384 * i); f12_store(out + 384 * i, cyclo ? f12_cyclo_sqr(a) : f12_sqr(a)); }
}
// pair-lane forms: Miller accumulator fed by the single-lane line phase, and the final exponentiation
void hc_pair_lanes(const uint8_t *P, const uint8_t *Q, size_t n, uint8_t *out, int do_final_exp) {
    for (size_t i = 0; i < n; i++) {
        const uint8_t *p = P + 64 * i, *q = Q + 128 * i;
        G1A a{fe_load(p), fe_load(p + 32)};
        G2A b{f2_load(q), f2_load(q + 64)};
        LineS lines[MILLER_LINES];
        int cnt = 0;
        miller_lines<true>(a, b, [&](const LineS &l) { lines[cnt++] = l; });
        PairRendezvous rv;
        auto lane = [&](bool odd) {
            PairHost x{odd, &rv};
            int k = 0;
            F6 h = miller_accumulate_pair(x, [&]() -> LineS { return lines[k++]; });
            if (do_final_exp) h = final_exp_pair(x, h);
            f6_store(out + 384 * i + (odd ? 192 : 0), h);
            stats_flush();
        };
        std::thread t1(lane, true);
        lane(false);
        t1.join();
    }
}
// The sparse line products of the lane-pair accumulators side by side on the same operands: the eight-product form (five at c0 = 1)
// and the doubled seven-product form (four).  H: n x 2 x 54 int32, the RAW limbs of a positive-normalised accumulator (even lane's
// half, then the odd lane's) — limbs 0..7 within [-2^4, 2^29 + 2^4], the value's sign in the top limb, |value| < 0.51 p: the class
// every step of miller_accumulate_pair ends in, so the extremes of that class can be put in directly.  L: n x 4 x 64 bytes, gnark
// E2 values (c0, c3, u, w) with c4 = u - w entering un-normalised, as a tangent's r2 = E - B does.  one = 0: f12p_mul_034<true> into
// out_old, f12p_mul_034_x2 into out_new; one = 1: f12p_mul_34<true> and f12p_mul_34_half on half the line (c0 is not read).  Canonical
// gnark bytes; the caller checks out_new = 2 out_old (one = 0) or out_new = out_old (one = 1).
static Fe fe_raw_pn(const int32_t *w) {
    Fe r;
    for (int i = 0; i < NL; i++) r.v[i] = w[i];
    constexpr double P8 = (double)f29_p(NL - 1);
    r.lo[0] = 0; r.hi[0] = (double)LMASK;
    for (int i = 1; i < NL - 1; i++) { r.lo[i] = -16; r.hi[i] = (double)LMASK + 16; }
    r.hi[NL - 1] = P8 / 2 + 270 + 16; r.lo[NL - 1] = -r.hi[NL - 1];
    r.vb = 0.51;
    check_limbs(r, "raw positive-normalised limb");
    return r;
}
static F6 f6_raw_pn(const int32_t *w) {
    return F6{F2{fe_raw_pn(w), fe_raw_pn(w + NL)}, F2{fe_raw_pn(w + 2 * NL), fe_raw_pn(w + 3 * NL)}, F2{fe_raw_pn(w + 4 * NL), fe_raw_pn(w + 5 * NL)}};
}
void hc_sparse_products(const int32_t *H, const uint8_t *L, size_t n, int one, uint8_t *out_old, uint8_t *out_new) {
    for (size_t i = 0; i < n; i++) {
        const uint8_t *l = L + 256 * i;
        const F2 c0 = f2_load(l), c3 = f2_load(l + 64), c4 = f2_sub(f2_load(l + 128), f2_load(l + 192));
        const F2 c0x2 = f2_norm(f2_dbl(c0));
        PairRendezvous rv;
        auto lane = [&](bool odd) {
            PairHost x{odd, &rv};
            const F6 h = f6_raw_pn(H + (2 * i + (odd ? 1 : 0)) * LINE_WORDS);
            const size_t o = 384 * i + (odd ? 192 : 0);
            f6_store(out_old + o, one ? f12p_mul_34<true>(x, h, c3, c4) : f12p_mul_034<true>(x, h, c0, c3, c4));
            f6_store(out_new + o, one ? f12p_mul_34_half(x, h, f2_halve(c3), f2_halve(f2_norm(c4))) : f12p_mul_034_x2(x, h, c0x2, c3, c4));
            stats_flush();
        };
        std::thread t1(lane, true);
        lane(false);
        t1.join();
    }
}
// product of the Miller functions of n pairs on ONE lane pair with shared squarings (k_miller_accumulate_chunks)
void hc_pair_lanes_multi(const uint8_t *P, const uint8_t *Q, size_t n, uint8_t *out) {
    std::vector<LineS> lines(n * MILLER_LINES);
    for (size_t i = 0; i < n; i++) {
        G1A a{fe_load(P + 64 * i), fe_load(P + 64 * i + 32)};
        G2A b{f2_load(Q + 128 * i), f2_load(Q + 128 * i + 64)};
        int cnt = 0;
        miller_lines(a, b, [&](const LineS &l) { lines[i * MILLER_LINES + cnt++] = l; });
    }
    PairRendezvous rv;
    auto lane = [&](bool odd) {
        PairHost x{odd, &rv};
        F6 h = miller_accumulate_multi(x, (int)n, [&](int p, int li) -> LineS { return lines[(size_t)p * MILLER_LINES + li]; });
        f6_store(out + (odd ? 192 : 0), h);
        stats_flush();
    };
    std::thread t1(lane, true);
    lane(false);
    t1.join();
}
// fixed-Q multi-pairing exactly as k_q_lines + k_q_lines_scale + k_g1_line_point + k_miller_accumulate_fixed_q do it: the RAW line
// coefficients of every Q_i (miller_lines_raw) scaled to c0 = 1, evaluated at (xP / 2yP, 1 / 2yP) inside the accumulator (one
// Fp x Fp2 product per lane, swapped), shared squarings on one lane pair; out = the Miller value of prod e(P_i, Q_i) up to a
// factor in Fp2 (do_final_exp = 0: the caller applies the final exponentiation, which removes it) or the GT value
void hc_pair_fixed_q(const uint8_t *P, const uint8_t *Q, size_t n, uint8_t *out, int do_final_exp) {
    std::vector<Line34> tab(n * MILLER_LINES);
    std::vector<G1A> pts(n);                                    // (x / 2y, 1 / 2y)
    for (size_t base = 0; base < n; base += 8)                  // k_g1_line_point: groups of 8 points share one inversion
        fe_batch_inverse<8>(n - base < 8 ? (int)(n - base) : 8, [&](int j) { return fe_load(P + 64 * (base + j) + 32); },
                            [&](int j, const Fe &y_inverse) { const Fe yinv = fe_halve(y_inverse); pts[base + j] = G1A{fe_mul(fe_load(P + 64 * (base + j)), yinv), yinv}; });
    for (size_t i = 0; i < n; i++) {
        G2A b{f2_load(Q + 128 * i), f2_load(Q + 128 * i + 64)};
        int cnt = 0;
        miller_lines_raw(b, [&](const LineE &l) {
            F2 inv = f2_inv(f2_norm(l.r0));
            tab[i * MILLER_LINES + cnt++] = Line34{f2_mul(f2_norm(l.r1), inv), f2_mul(f2_norm(l.r2), inv)};
        });
    }
    PairRendezvous rv;
    auto lane = [&](bool odd) {
        PairHost x{odd, &rv};
        F6 h = miller_accumulate_multi_34(x, (int)n, [&](int p, int li) -> Line34 {
            const Line34 &r = tab[(size_t)p * MILLER_LINES + li];
            const F2 mine = f2_mul_fe(x.odd ? r.c4 : r.c3, x.odd ? pts[p].y : pts[p].x), other = x.swap(mine);   // one product per lane, swapped
            return Line34{x.odd ? other : mine, x.odd ? mine : other};
        });
        if (do_final_exp) h = final_exp_pair(x, h);
        f6_store(out + (odd ? 192 : 0), h);
        stats_flush();
    };
    std::thread t1(lane, true);
    lane(false);
    t1.join();
}
void hc_gt_pair_ops(const uint8_t *A, const uint8_t *B, size_t n, uint8_t *mul, uint8_t *sqr, uint8_t *csqr, uint8_t *inv, uint8_t *frob1) {
    for (size_t i = 0; i < n; i++) {
        PairRendezvous rv;
        auto lane = [&](bool odd) {
            PairHost x{odd, &rv};
            size_t o = 384 * i + (odd ? 192 : 0);
            F6 a = f6_load(A + o), b = f6_load(B + o);
            f6_store(mul + o, f12p_mul(x, a, b));
            f6_store(sqr + o, f12p_sqr(x, a));
            f6_store(csqr + o, f12p_cyclo_sqr<true>(x, a));
            f6_store(inv + o, f12p_inv(x, a));
            f6_store(frob1 + o, f12p_frob(x, a, 1));
            stats_flush();
        };
        std::thread t1(lane, true);
        lane(false);
        t1.join();
    }
}
// GT.Exp on a lane pair (k_gt_exp): out = a^k for 256-bit little-endian k
void hc_gt_exp_pair(const uint8_t *A, const uint8_t *K, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; i++) {
        PairRendezvous rv;
        uint32_t k[8]; memcpy(k, K + 32 * i, 32);
        auto lane = [&](bool odd) {
            PairHost x{odd, &rv};
            size_t o = 384 * i + (odd ? 192 : 0);
            alignas(16) int32_t tab[GT_EXP_TAB_DWORDS];
            f6_store(out + o, f12p_exp256(x, f6_load(A + o), k, tab));
            stats_flush();
        };
        std::thread t1(lane, true);
        lane(false);
        t1.join();
    }
}
// The final exponentiation of the lane-pair form (k_final_exp: final_exp_pair) and of the latency form (k_final_exp_wide:
// wide_final_exp) on ANY Fp12 value, as gpbc_final_exp hands it over: zero, one, subfield elements and elements already in GT
// included, which no Miller loop produces (hc_pair_lanes / hc_pair_wide reach these functions only behind one).
void hc_final_exp_forms(const uint8_t *F, size_t n, uint8_t *out, int wide) {
    for (size_t i = 0; i < n; i++) {
        if (wide) {
            WideHost m;
            for (int c = 0; c < 6; c++) m.s[wv(0) + c] = f2_load(F + 384 * i + 64 * c);
            wide_final_exp(m);
            for (int c = 0; c < 6; c++) f2_store(out + 384 * i + 64 * c, m.s[c]);
            stats_flush();
            continue;
        }
        PairRendezvous rv;
        auto lane = [&](bool odd) {
            PairHost x{odd, &rv};
            size_t o = 384 * i + (odd ? 192 : 0);
            f6_store(out + o, final_exp_pair(x, f6_load(F + o)));
            stats_flush();
        };
        std::thread t1(lane, true);
        lane(false);
        t1.join();
    }
}
// The predicate that chooses the squarings of GT.Exp, as each form answers it: out[3 i] the even lane's and out[3 i + 1] the odd
// lane's f12p_is_cyclotomic (documented to be the same on both), out[3 i + 2] wide_is_cyclotomic with the scratch values wide_exp256 gives it
void hc_gt_is_cyclotomic(const uint8_t *A, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; i++) {
        PairRendezvous rv;
        auto lane = [&](bool odd) {
            PairHost x{odd, &rv};
            out[3 * i + (odd ? 1 : 0)] = f12p_is_cyclotomic(x, f6_load(A + 384 * i + (odd ? 192 : 0))) ? 1 : 0;
            stats_flush();
        };
        std::thread t1(lane, true);
        lane(false);
        t1.join();
        WideHost m;
        for (int c = 0; c < 6; c++) m.s[wv(1) + c] = f2_load(A + 384 * i + 64 * c);
        out[3 * i + 2] = wide_is_cyclotomic(m, wv(1), wv(8), wv(9)) ? 1 : 0;
        stats_flush();
    }
}
// segmented GT multi-exponentiation exactly as gpbc_gt_multi_exp_dev (csrc/gpbc_gtmexp.hip) runs it: the plan and the level walk of
// csrc/segred29.hip.hpp with GT_MEXP_SHAPE (segred_piece per piece, the function the kernel calls, so a table is clamped as on the
// device; the value buffers sized by segred_plan), the same lane functions (f12p_multi_exp, f12p_product for K = null and for the
// folds), one piece per lane pair.  out[s] = prod_{i in [seg_off[s], seg_off[s+1])} A[i]^K[i]; nk = n, or one list of nk exponents for all segments
void hc_gt_multi_exp_pair(const uint8_t *A, const uint8_t *K, size_t nk, const uint64_t *seg_off, size_t n, size_t n_seg, uint8_t *out) {
    const SegRedPlan plan = segred_plan(GT_MEXP_SHAPE, 384, GT_MEXP_TAB_BYTES, n, n_seg, K != nullptr);
    std::vector<uint8_t> v0(plan.val_bytes[0]), v1(plan.val_bytes[1]);
    uint8_t *const val[2] = {v0.data(), v1.data()};
    segred_walk(GT_MEXP_SHAPE, segred_args(A, K, nk, seg_off, n, n_seg), val, out, [&](SegRedArgs g, size_t pieces) {
        g.n_pieces = pieces;
        for (size_t pair = 0; pair < pieces; pair++) {
            size_t lo, a, b, P;
            segred_piece(g, pair, lo, a, b, P);
            PairRendezvous rv;
            auto lane = [&](bool odd) {
                PairHost px{odd, &rv};
                const size_t half = odd ? 192 : 0, k0 = g.k_shared ? lo : 0;
                auto base = [&](size_t i) { return f6_load(g.x + (a + i) * 384 + half); };
                F6 r;
                if (g.k) {
                    alignas(16) static thread_local int32_t tab[GT_MEXP_TAB_DWORDS];
                    r = f12p_multi_exp(px, b - a, base, [&](size_t i, int w) { uint32_t d; memcpy(&d, g.k + 32 * (a + i - k0) + 4 * (w >> 3), 4); return (int)((d >> (4 * (w & 7))) & 15); }, tab);
                } else r = f12p_product(px, b - a, base);
                f6_store(g.out + P * 384 + half, r);
                stats_flush();
            };
            std::thread t1(lane, true);
            lane(false);
            t1.join();
        }
        return 0;
    });
}
// wire formats (csrc/wire29.hip.hpp): kind 0 G1, 1 G2, 2 GT; the same per-element functions the kernels call
void hc_wire_encode(int kind, const uint8_t *in, size_t n, int compressed, uint8_t *out) {
    for (size_t i = 0; i < n; i++) {
        if (kind == 0) g1_wire_encode(out + i * (compressed ? 32 : 64), in + 64 * i, compressed != 0);
        else if (kind == 1) g2_wire_encode(out + i * (compressed ? 64 : 128), in + 128 * i, compressed != 0);
        else gt_wire_encode(out + 384 * i, in + 384 * i);
    }
}
void hc_wire_decode(int kind, const uint8_t *in, int elem_bytes, size_t n, uint8_t *out, uint8_t *ok) {
    for (size_t i = 0; i < n; i++) {
        if (kind == 0) ok[i] = g1_wire_decode(out + 64 * i, in + (size_t)elem_bytes * i, elem_bytes);
        else if (kind == 1) ok[i] = g2_wire_decode(out + 128 * i, in + (size_t)elem_bytes * i, elem_bytes);
        else ok[i] = gt_wire_decode(out + 384 * i, in + 384 * i);
    }
}
// the transcript hash and the plain SHA-256 (csrc/transcript29.hip.hpp): the lane functions of k_hash_g1_gt_gt_to_fr and k_sha256, one
// item after the other; the offsets go through msg_range as in the kernel (total = the length of the message buffer)
void hc_hash_g1_gt_gt_to_fr(const uint8_t *u, const uint8_t *v, const uint8_t *w, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; i++) hash_g1_gt_gt_to_fr_lane(u + 64 * i, v + 384 * i, w + 384 * i, out + 32 * i);
    stats_flush();
}
void hc_sha256(const uint8_t *msgs, const uint64_t *off, size_t total, size_t n, int to_fr, uint8_t *out) {
    for (size_t i = 0; i < n; i++) {
        uint64_t lo, len;
        msg_range(off, total, i, lo, len);
        sha256_lane(msgs + lo, len, to_fr != 0, out + 32 * i);
    }
    stats_flush();
}
// the square roots of csrc/wire29.hip.hpp on their own (gnark fp.Element / E2 in and out): out = the value returned, ok = whether it is a root
void hc_fe_sqrt(const uint8_t *A, size_t n, uint8_t *out, uint8_t *ok) {
    for (size_t i = 0; i < n; i++) { bool good; fe_store(out + 32 * i, fe_sqrt(fe_load(A + 32 * i), good)); ok[i] = good ? 1 : 0; }
}
void hc_f2_sqrt(const uint8_t *A, size_t n, uint8_t *out, uint8_t *ok) {
    for (size_t i = 0; i < n; i++) { bool good; f2_store(out + 64 * i, f2_sqrt(f2_load(A + 64 * i), good)); ok[i] = good ? 1 : 0; }
}
// hash to curve, group part (csrc/h2c29.hip.hpp): U = n x 2 field elements (gnark fp.Element / E2), out = n affine points
void hc_map_fields(int g2, const uint8_t *U, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; i++) {
        if (!g2) {
            AffP<Fe> r;
            g1_map_fields(r, fe_load(U + 64 * i), fe_load(U + 64 * i + 32));
            fe_store(out + 64 * i, r.x); fe_store(out + 64 * i + 32, r.y);
        } else {
            AffP<F2> r;
            g2_map_fields(r, f2_load(U + 128 * i), f2_load(U + 128 * i + 64));
            f2_store(out + 128 * i, r.x); f2_store(out + 128 * i + 64, r.y);
        }
    }
}
// fixed-base MSM exactly as k_g1_fb_build / k_g1_fb_msm do it (G1): 8-bit window table of every base, then 32 mixed
// additions per term; out[m] = sum_j [K[m][j]] B[j]
void hc_g1_fb_msm(const uint8_t *B, size_t nbase, const uint8_t *K, size_t n_msm, uint8_t *out) {
    const size_t E = 32 * 255;
    std::vector<int32_t> table(nbase * E * 32 + 4);
    int32_t *tb0 = table.data();
    while (((uintptr_t)tb0) & 15) tb0++;
    std::vector<uint8_t> inf(nbase);
    for (size_t b = 0; b < nbase; b++) {
        AffP<Fe> base{fe_load(B + 64 * b), fe_load(B + 64 * b + 32), bytes_all_zero(B + 64 * b, 16)};
        inf[b] = base.inf;
        for (int w = 0; w < 32; w++)
            for (int d = 1; d <= 255; d += (w % 5 == 0 || d < 4 || d > 252) ? 1 : 37) {     // a subset of the rows is enough for the bounds proof
                uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                k[w >> 2] = (uint32_t)d << (8 * (w & 3));
                alignas(16) int32_t tab[glv_table_dwords<Fe>()];
                JacP<Fe> r; scalar_mul29_jac<Fe>(r, base, k, tab);
                AffP<Fe> a; jac_to_affine(a, r);
                tab_store(tb0 + ((b * 32 + w) * 255 + d - 1) * 32, 0, a);
            }
    }
    for (size_t m = 0; m < n_msm; m++) {
        JacP<Fe> acc; jac_set_inf(acc);
        for (size_t j = 0; j < nbase; j++) {
            if (inf[j]) continue;
            uint32_t k[8]; memcpy(k, K + 32 * (m * nbase + j), 32);
            for (int w = 0; w < 32; w++) {
                int d = (k[w >> 2] >> (8 * (w & 3))) & 255;
                if (!d) continue;
                AffP<Fe> e; tab_load(tb0 + ((j * 32 + w) * 255 + d - 1) * 32, 0, e);
                jac_add_mixed(acc, acc, e);
            }
        }
        AffP<Fe> a; jac_to_affine(a, acc);
        fe_store(out + 64 * m, a.x); fe_store(out + 64 * m + 32, a.y);
    }
}
int hc_group_op(int is_g2, int op, const uint8_t *A, const uint8_t *B, size_t nb, size_t n, uint8_t *out, int k) {
    if (op < 0 || op > 2 || (op != GROUP_DBL && nb != 1 && nb != n)) return -1;
    if (k == 0) k = is_g2 ? GROUP_K_G2 : GROUP_K_G1;
    switch (k * 2 + (is_g2 ? 1 : 0)) {
        case 2: group_host<Fe, 1>(op, A, B, nb, n, out); break;
        case 3: group_host<F2, 1>(op, A, B, nb, n, out); break;
        case 8: group_host<Fe, 4>(op, A, B, nb, n, out); break;
        case 9: group_host<F2, 4>(op, A, B, nb, n, out); break;
        case 12: group_host<Fe, 6>(op, A, B, nb, n, out); break;
        case 13: group_host<F2, 6>(op, A, B, nb, n, out); break;
        case 16: group_host<Fe, 8>(op, A, B, nb, n, out); break;
        case 17: group_host<F2, 8>(op, A, B, nb, n, out); break;
        default: return -1;
    }
    stats_flush();
    return 0;
}
int hc_group_k(int is_g2) { return is_g2 ? GROUP_K_G2 : GROUP_K_G1; }
void hc_msm(int g2, const uint8_t *B, const uint8_t *K, size_t n, int c, uint8_t *out) {
    if (!g2) msm_host<Fe>(B, K, n, c, out, 64,
                          [](const uint8_t *p) { return AffP<Fe>{fe_load(p), fe_load(p + 32), bytes_all_zero(p, 16)}; },
                          [](uint8_t *p, const AffP<Fe> &r) { fe_store(p, r.x); fe_store(p + 32, r.y); });
    else msm_host<F2>(B, K, n, c, out, 128,
                      [](const uint8_t *p) { return AffP<F2>{f2_load(p), f2_load(p + 64), bytes_all_zero(p, 32)}; },
                      [](uint8_t *p, const AffP<F2> &r) { f2_store(p, r.x); f2_store(p + 64, r.y); });
}
// The scalar field (csrc/fr29.hip.hpp) exactly as the kernels of csrc/gpbc_fr.hip run it.  op: FrOp, or FR_OPS = the inversion, whose
// lanes own k elements each (k = 0: the kernel's FR_INV_K) at t, t + T, ... with T = ceil(n / k)
int hc_fr_op(int op, const uint8_t *A, const uint8_t *B, size_t nb, size_t n, uint8_t *out, int k) {
    if (op < 0 || op > FR_OPS || (op <= FR_MUL && nb != 1 && nb != n)) return -1;
    const size_t step = nb == n ? 32 : 0;
    if (op == FR_OPS) {
        switch (k ? k : FR_INV_K) {
            case 1: fr_inverse_host<1>(A, n, out); break;
            case 4: fr_inverse_host<4>(A, n, out); break;
            case 8: fr_inverse_host<8>(A, n, out); break;
            default: return -1;
        }
    } else {
        for (size_t i = 0; i < n; i++) {
            const uint8_t *a = A + 32 * i, *b = op <= FR_MUL ? B + i * step : a;
            switch (op) {
                case FR_ADD: fr_op_lane<FR_ADD>(a, b, out + 32 * i); break;
                case FR_SUB: fr_op_lane<FR_SUB>(a, b, out + 32 * i); break;
                case FR_MUL: fr_op_lane<FR_MUL>(a, b, out + 32 * i); break;
                case FR_NEG: fr_op_lane<FR_NEG>(a, b, out + 32 * i); break;
                case FR_FROM_MONT: fr_op_lane<FR_FROM_MONT>(a, b, out + 32 * i); break;
                default: fr_op_lane<FR_TO_MONT>(a, b, out + 32 * i); break;
            }
        }
    }
    stats_flush();
    return 0;
}
int hc_fr_inv_k(void) { return FR_INV_K; }
// k_fr_poly_from_roots: per root, every coefficient up to the new degree from itself and its lower neighbour (all read, then all written)
int hc_fr_poly_from_roots(const uint8_t *roots, size_t B, size_t k, uint8_t *coeffs_out) {
    if (B < 1 || B > (size_t)FR_POLY_MAX_B) return -1;
    std::vector<Fr> cs(B + 1), nw(B + 1);
    for (size_t j = 0; j < k; j++) {
        for (size_t i = 0; i <= B; i++) cs[i] = i ? fr_zero() : fr_plain_one();
        for (size_t s = 0; s < B; s++) {
            const Fr nr = fr_poly_neg_root(roots + (j * B + s) * 32);
            for (size_t i = 0; i <= s + 1; i++) nw[i] = fr_poly_root_step(i ? cs[i - 1] : fr_zero(), cs[i], nr);
            for (size_t i = 0; i <= s + 1; i++) cs[i] = nw[i];
        }
        for (size_t i = 0; i <= B; i++) fr_poly_store(coeffs_out + (j * (B + 1) + i) * 32, cs[i]);
    }
    stats_flush();
    return 0;
}
// k_fr_poly_quotients: one walk from the top coefficient down per (polynomial, point); rows of `stride` scalars
int hc_fr_poly_quotients(const uint8_t *coeffs, const uint8_t *points, size_t B, size_t k, size_t stride, uint8_t *q_out, uint8_t *ok_out) {
    if (B < 1 || B > (size_t)FR_POLY_MAX_B || stride < B) return -1;
    std::vector<Fr> cs(B + 1);
    for (size_t j = 0; j < k; j++) {
        for (size_t i = 0; i <= B; i++) cs[i] = fr_poly_coeff_in(coeffs + (j * (B + 1) + i) * 32);
        for (size_t pi = 0; pi < B; pi++) {
            const Fr point = fr_poly_point(points + (j * B + pi) * 32);
            uint8_t *row = q_out + (j * B + pi) * stride * 32;
            Fr carry = fr_zero();
            for (size_t c = B; c-- > 0;) {
                carry = fr_poly_horner_step(carry, cs[c + 1], point);
                fr_store_canonical(row + 32 * c, carry);
            }
            const bool ok = fr_limbs_zero(fr_poly_horner_step(carry, cs[0], point));
            ok_out[j * B + pi] = ok ? 1 : 0;
            memset(row + (ok ? B * 32 : 0), 0, (stride - (ok ? B : 0)) * 32);
        }
    }
    stats_flush();
    return 0;
}
int hc_fr_lagrange_basis(const uint8_t *set, size_t n_set_rows, size_t B, const uint8_t *nodes, size_t n_node_rows, size_t m, const uint8_t *x, size_t nx, size_t k,
                         uint8_t *out, int g) {
    if (B < 1 || B > (size_t)FR_POLY_MAX_B || m < 1 || m > (size_t)FR_POLY_MAX_B) return -1;
    if (k && ((n_set_rows != 1 && n_set_rows != k) || (nodes ? n_node_rows != 1 && n_node_rows != k : m != B) || (x ? nx != 1 && nx != k : nx != 0))) return -1;
    switch (g ? g : FR_LAGRANGE_G) {
        case 1: fr_lagrange_host<1>(set, n_set_rows, B, nodes, n_node_rows, m, x, nx, k, out); break;
        case 4: fr_lagrange_host<4>(set, n_set_rows, B, nodes, n_node_rows, m, x, nx, k, out); break;
        default: return -1;
    }
    stats_flush();
    return 0;
}
int hc_fr_lagrange_g(void) { return FR_LAGRANGE_G; }
// k_fr_lagrange_basis as it is LAUNCHED: the geometry, the staging and the lane mapping of fr29.hip.hpp, workgroup by workgroup, on a
// stand-in for the LDS block that refuses a store outside the block or over another element and a load of anything but a whole
// staged element.  geom_out: [gpr, rpb, bpr, large, workgroups, active lanes].  Returns -2 on such a refusal.
int hc_fr_lagrange_launch(const uint8_t *set, size_t n_set_rows, size_t B, const uint8_t *nodes, size_t n_node_rows, size_t m, const uint8_t *x, size_t nx, size_t k,
                          uint8_t *out, uint32_t *geom_out) {
    if (B < 1 || B > (size_t)FR_POLY_MAX_B || m < 1 || m > (size_t)FR_POLY_MAX_B || !k) return -1;
    if ((n_set_rows != 1 && n_set_rows != k) || (nodes ? n_node_rows != 1 && n_node_rows != k : m != B) || (x ? nx != 1 && nx != k : nx != 0)) return -1;
    const bool shared_set = n_set_rows == 1 && k > 1;
    const LagrangeGeom g = fr_lagrange_geometry(B, m, shared_set);
    const size_t set_step = shared_set ? 0 : B * 32, node_step = nodes && n_node_rows == k && k > 1 ? m * 32 : 0, x_step = x && nx == k && k > 1 ? 32 : 0;
    const size_t words = (size_t)(g.large ? FR_LAG_LARGE : FR_LAG_SMALL) * NL + FR_LAG_WAVE, grid = fr_lagrange_grid(g, k);
    std::vector<Fr> lds(words);
    std::vector<int64_t> owner(words);
    bool bad = false;
    uint32_t active = 0;
    for (size_t block = 0; block < grid; block++) {
        std::fill(owner.begin(), owner.end(), -1);
        for (uint32_t lane = 0; lane < FR_LAG_WAVE; lane++)
            fr_lagrange_stage(g, (uint32_t)block, lane, k, set, set_step, [&](uint32_t off, const Fr &v) {
                if ((size_t)off + NL > words) { bad = true; return; }
                for (int i = 0; i < NL; i++) { if (owner[off + i] != -1) bad = true; owner[off + i] = off; }
                lds[off] = v;
            });
        for (uint32_t lane = 0; lane < FR_LAG_WAVE && !bad; lane++) {
            const LagrangeLane l = fr_lagrange_map(g, (uint32_t)block, lane, k);
            if (!l.active) continue;
            if (l.row >= k) { bad = true; break; }
            active++;
            const uint32_t mine = set_step ? l.lr * fr_lagrange_pitch(g) : 0u;
            const Fr xc = x ? fr_lagrange_in(x + l.row * x_step) : fr_zero();
            fr_lagrange_lane<FR_LAGRANGE_G>([&](uint32_t u) {
                const size_t off = mine + (size_t)u * NL;
                if (off + NL > words || owner[off] != (int64_t)off) { bad = true; return fr_zero(); }
                return lds[off];
            }, g.B, nodes ? nodes + l.row * node_step : nullptr, xc, g.m, l.gi, g.gpr, out + l.row * g.m * 32);
        }
        if (bad) return -2;
    }
    if (geom_out) { geom_out[0] = g.gpr; geom_out[1] = g.rpb; geom_out[2] = g.bpr; geom_out[3] = g.large; geom_out[4] = (uint32_t)grid; geom_out[5] = active; }
    stats_flush();
    return 0;
}
static bool fr_lsss_bad_args(const void *matrix, size_t n_matrices, size_t rows, size_t cols, const void *held, size_t k) {
    return rows < 1 || rows > (size_t)FR_LSSS_MAX || cols < 1 || cols > (size_t)FR_LSSS_MAX || !k || (n_matrices != 1 && n_matrices != k) || !matrix || !held;
}
// the lane functions on one system at a time (a wave of its own, whatever the launch would share)
int hc_fr_lsss_weights(const uint8_t *matrix, size_t n_matrices, size_t rows, size_t cols, const uint8_t *held, size_t k, uint8_t *w_out, uint8_t *ok_out) {
    if (fr_lsss_bad_args(matrix, n_matrices, rows, cols, held, k)) return -1;
    LsssGeom g = fr_lsss_geometry(rows, cols);
    g.spw = 1;
    std::vector<Fr> lds(g.sys_words);
    for (size_t t = 0; t < k; t++)
        fr_lsss_block(g, 0, 1, matrix + (n_matrices == 1 ? 0 : t) * rows * cols * 32, 0, held + t * rows, [&](uint32_t off) { return lds[off]; },
                      [&](uint32_t off, const Fr &v) { lds[off] = v; }, w_out + t * rows * 32, ok_out + t, nullptr);
    stats_flush();
    return 0;
}
// k_fr_lsss_weights as it is LAUNCHED: geometry, staging and lane mapping workgroup by workgroup on a stand-in for the LDS block of the
// instance the launch would take, which refuses a store outside the block or across element boundaries and a load of anything but a
// whole element stored before.  geom_out: [gw, spw, pitch, sys_words, LDS instance, workgroups, lanes that own a weight].  -2 on a refusal.
int hc_fr_lsss_launch(const uint8_t *matrix, size_t n_matrices, size_t rows, size_t cols, const uint8_t *held, size_t k, uint8_t *w_out, uint8_t *ok_out, uint32_t *geom_out) {
    if (fr_lsss_bad_args(matrix, n_matrices, rows, cols, held, k)) return -1;
    const LsssGeom g = fr_lsss_geometry(rows, cols);
    const size_t mat_step = n_matrices == 1 && k > 1 ? 0 : rows * cols * 32;
    const size_t words = (size_t)fr_lsss_words(g.level), grid = fr_lsss_grid(g, k);
    std::vector<Fr> lds(words);
    std::vector<int64_t> owner(words);
    bool bad = false;
    uint32_t active = 0;
    for (size_t block = 0; block < grid && !bad; block++) {
        std::fill(owner.begin(), owner.end(), -1);
        fr_lsss_block(g, (uint32_t)block, k, matrix, mat_step, held,
                      [&](uint32_t off) {
                          if ((size_t)off + NL > words || owner[off] != (int64_t)off) { bad = true; return fr_zero(); }
                          return lds[off];
                      },
                      [&](uint32_t off, const Fr &v) {
                          if ((size_t)off + NL > words) { bad = true; return; }
                          for (int i = 0; i < NL; i++) { if (owner[off + i] != -1 && owner[off + i] != (int64_t)off) bad = true; owner[off + i] = off; }
                          lds[off] = v;
                      },
                      w_out, ok_out, &active);
    }
    if (bad) return -2;
    if (geom_out) { geom_out[0] = g.gw; geom_out[1] = g.spw; geom_out[2] = g.pitch; geom_out[3] = g.sys_words; geom_out[4] = g.level; geom_out[5] = (uint32_t)grid; geom_out[6] = active; }
    stats_flush();
    return 0;
}
// A stand-in for an LDS block of `words` words, elements of NL words and single words side by side (the kernels as they are LAUNCHED,
// below; the single words are k_fr_tree_weights' and k_fr_forest_weights').  A store outside the block, an element across a word or
// another element's boundaries, a word inside an element, and a load of anything but what was stored whole at that offset are refused.
struct CheckedLds {
    std::vector<Fr> v;
    std::vector<uint32_t> w;
    std::vector<int64_t> owner;                 // -1 free, off: a word of the element at off, -2 - off: the single word at off
    bool bad = false;
    explicit CheckedLds(size_t words) : v(words), w(words, 0), owner(words, -1) {}
    void reset() { std::fill(owner.begin(), owner.end(), -1); }
    Fr get(uint32_t off) {
        if ((size_t)off + NL > v.size() || owner[off] != (int64_t)off) { bad = true; return fr_zero(); }
        return v[off];
    }
    void put(uint32_t off, const Fr &x) {
        if ((size_t)off + NL > v.size()) { bad = true; return; }
        for (int i = 0; i < NL; i++) { if (owner[off + i] != -1 && owner[off + i] != (int64_t)off) bad = true; owner[off + i] = off; }
        v[off] = x;
    }
    uint32_t getw(uint32_t off) {
        if ((size_t)off >= w.size() || owner[off] != -2 - (int64_t)off) { bad = true; return 0; }
        return w[off];
    }
    void putw(uint32_t off, uint32_t x) {
        if ((size_t)off >= w.size() || (owner[off] != -1 && owner[off] != -2 - (int64_t)off)) { bad = true; return; }
        owner[off] = -2 - (int64_t)off;
        w[off] = x;
    }
};
// k_fr_poly_eval as it is launched: geometry, staging and lane mapping of share29.hip.hpp, workgroup by workgroup.
// geom_out: [rpb, bpr, large, workgroups, active lanes].  -1: arguments the entry refuses; -2: a refusal of the LDS stand-in or a lane outside the rows.
int hc_fr_poly_eval(const uint8_t *coeffs, size_t n_coeff_rows, size_t d, const uint8_t *points, size_t n_point_rows, size_t m, size_t k, uint8_t *out, uint32_t *geom_out) {
    if (d < 1 || d > (size_t)FR_POLY_MAX_B || m < 1 || m > (size_t)FR_POLY_MAX_B || !k) return -1;
    if ((n_coeff_rows != 1 && n_coeff_rows != k) || (n_point_rows != 1 && n_point_rows != k) || !coeffs || !points || !out) return -1;
    const bool shared = n_coeff_rows == 1 && k > 1;
    const PolyEvalGeom g = fr_poly_eval_geometry(d, m, shared);
    const size_t coeff_step = shared ? 0 : d * 32, point_step = n_point_rows == k && k > 1 ? m * 32 : 0;
    CheckedLds lds((size_t)(g.large ? FR_EVAL_LARGE : FR_EVAL_SMALL) * NL + FR_SHARE_WAVE);
    const size_t grid = fr_poly_eval_grid(g, k);
    uint32_t active = 0;
    for (size_t block = 0; block < grid; block++) {
        lds.reset();
        for (uint32_t lane = 0; lane < FR_SHARE_WAVE; lane++)
            fr_poly_eval_stage(g, (uint32_t)block, lane, k, coeffs, coeff_step, [&](uint32_t off, const Fr &v) { lds.put(off, v); });
        for (uint32_t lane = 0; lane < FR_SHARE_WAVE && !lds.bad; lane++) {
            const PolyEvalLane l = fr_poly_eval_map(g, (uint32_t)block, lane, k);
            if (!l.active) continue;
            if (l.row >= k || l.t >= m) return -2;
            active++;
            const uint32_t mine = coeff_step ? l.lr * fr_poly_eval_pitch(g) : 0u;
            fr_poly_eval_lane([&](uint32_t i) { return lds.get(mine + i * NL); }, g.d, points + l.row * point_step + 32 * (size_t)l.t, out + 32 * (l.row * g.m + l.t));
        }
        if (lds.bad) return -2;
    }
    if (geom_out) { geom_out[0] = g.rpb; geom_out[1] = g.bpr; geom_out[2] = g.large; geom_out[3] = (uint32_t)grid; geom_out[4] = active; }
    stats_flush();
    return 0;
}
// the plan of a node list alone: sizes_out [L, G, C, depth, narrowest level, units]; -1 and the reason in why (up to 96 bytes) when it is refused
int hc_fr_share_plan(const uint32_t *nodes, size_t n_nodes, uint32_t *sizes_out, char *why) {
    SharePlan p;
    const char *w = fr_share_plan(reinterpret_cast<const ShareNode *>(nodes), n_nodes, p);
    if (w) { if (why) snprintf(why, 96, "%s", w); return -1; }
    if (sizes_out) { sizes_out[0] = p.L; sizes_out[1] = p.G; sizes_out[2] = p.C; sizes_out[3] = p.depth; sizes_out[4] = p.wmin; sizes_out[5] = (uint32_t)p.units.size(); }
    return 0;
}
// k_fr_share_tree as it is launched: the plan, the geometry, the staging and every level of share29.hip.hpp, workgroup by workgroup, a
// barrier = the end of a loop over the lanes.  geom_out: [L, G, C, depth, ipb, large, workgroups].  -1: a refused tree or argument; -2 as above, or a plan index outside its table.
int hc_fr_share_tree(const uint32_t *nodes, size_t n_nodes, const uint8_t *secrets, const uint8_t *coeffs, size_t k, uint8_t *out, uint32_t *geom_out) {
    SharePlan p;
    if (fr_share_plan(reinterpret_cast<const ShareNode *>(nodes), n_nodes, p) || !k || !secrets || !out || (p.C && !coeffs)) return -1;
    if (!fr_share_plan_ok(p)) return -2;
    const ShareGeom g = fr_share_geometry(p);
    CheckedLds lds((size_t)(g.large ? FR_TREE_LARGE : FR_TREE_SMALL) * NL + FR_SHARE_WAVE);
    const size_t grid = fr_share_grid(g, k);
    const auto get = [&](uint32_t off) { return lds.get(off); };
    const auto put = [&](uint32_t off, const Fr &v) { lds.put(off, v); };
    for (size_t block = 0; block < grid; block++) {
        lds.reset();
        if (!g.G) {
            for (uint32_t lane = 0; lane < FR_SHARE_WAVE; lane++) fr_share_single((uint32_t)block, lane, k, secrets, out);
            continue;
        }
        for (uint32_t lane = 0; lane < FR_SHARE_WAVE; lane++) fr_share_stage(g, (uint32_t)block, lane, k, secrets, coeffs, put);
        for (uint32_t lv = 1; lv <= g.depth && !lds.bad; lv++)
            for (uint32_t lane = 0; lane < FR_SHARE_WAVE; lane++) fr_share_level(g, p.units.data(), p.level_off.data(), lv, (uint32_t)block, lane, k, get, put, out);
        if (lds.bad) return -2;
    }
    if (geom_out) { geom_out[0] = g.L; geom_out[1] = g.G; geom_out[2] = g.C; geom_out[3] = g.depth; geom_out[4] = g.ipb; geom_out[5] = g.large; geom_out[6] = (uint32_t)grid; }
    stats_flush();
    return 0;
}
// k_fr_tree_weights as it is launched: the plan, the geometry, the staging and both passes of recon29.hip.hpp, workgroup by workgroup, a
// barrier = the end of a loop over the lanes.  geom_out: [L, G, U, depth, ipb, pitch, large, workgroups].  -1: a refused tree or argument;
// -2: a refusal of the LDS stand-in, a plan index outside its table or an output outside the rows.
int hc_fr_tree_weights(const uint32_t *nodes, size_t n_nodes, const uint8_t *held, size_t k, uint8_t *w_out, uint8_t *ok_out, uint32_t *geom_out) {
    ReconPlan p;
    if (fr_recon_plan(reinterpret_cast<const ShareNode *>(nodes), n_nodes, p) || !k || !held || !w_out || !ok_out) return -1;
    const ReconGeom g = fr_recon_geometry(p);
    if (g.G && (size_t)g.ipb * g.pitch > (size_t)(g.large ? FR_RECON_LARGE : FR_RECON_SMALL)) return -2;
    if (!fr_recon_plan_ok(p)) return -2;
    CheckedLds lds((size_t)(g.large ? FR_RECON_LARGE : FR_RECON_SMALL) + FR_RECON_WAVE);
    const size_t grid = fr_recon_grid(g, k);
    const auto get = [&](uint32_t off) { return lds.get(off); };
    const auto put = [&](uint32_t off, const Fr &v) { lds.put(off, v); };
    const auto getw = [&](uint32_t off) { return lds.getw(off); };
    const auto putw = [&](uint32_t off, uint32_t v) { lds.putw(off, v); };
    for (size_t block = 0; block < grid; block++) {
        lds.reset();
        if (!g.G) {
            for (uint32_t lane = 0; lane < FR_RECON_WAVE; lane++) fr_recon_single((uint32_t)block, lane, k, held, w_out, ok_out);
            continue;
        }
        for (uint32_t lane = 0; lane < FR_RECON_WAVE; lane++) fr_recon_stage(g, p.units.data(), (uint32_t)block, lane, k, held, put, putw);
        for (uint32_t lv = g.depth; lv-- > 0 && !lds.bad;)
            for (uint32_t lane = 0; lane < FR_RECON_WAVE; lane++) fr_recon_up(g, p.gates.data(), p.gate_off.data(), lv, (uint32_t)block, lane, k, getw, putw, ok_out);
        for (uint32_t lv = 1; lv <= g.depth && !lds.bad; lv++)
            for (uint32_t lane = 0; lane < FR_RECON_WAVE; lane++)
                fr_recon_down<FR_RECON_G>(g, p.units.data(), p.level_off.data(), lv, (uint32_t)block, lane, k, get, put, getw, putw, w_out);
        if (lds.bad) return -2;
    }
    if (geom_out) { geom_out[0] = g.L; geom_out[1] = g.G; geom_out[2] = g.U; geom_out[3] = g.depth; geom_out[4] = g.ipb; geom_out[5] = g.pitch; geom_out[6] = g.large; geom_out[7] = (uint32_t)grid; }
    stats_flush();
    return 0;
}
// k_fr_lsss_shares as it is launched: geometry, staging of the one matrix's row group and lane mapping of lsss29.hip.hpp, workgroup by
// workgroup.  geom_out: [rg, nrg, ipb, pitch, workgroups, active lanes].  -1: arguments the entry refuses; -2: a refusal of the LDS
// stand-in or a lane outside the outputs.
int hc_fr_lsss_shares(const uint8_t *matrix, size_t n_matrices, size_t rows, size_t cols, const uint8_t *vectors, size_t k, uint8_t *out, uint32_t *geom_out) {
    if (rows < 1 || rows > (size_t)FR_LSSS_MAX || cols < 1 || cols > (size_t)FR_LSSS_MAX || !k || (n_matrices != 1 && n_matrices != k) || !matrix || !vectors || !out) return -1;
    const bool shared = n_matrices == 1 && k > 1;
    const LsssSharesGeom g = fr_lsss_shares_geometry(rows, cols, shared);
    const size_t mat_step = shared ? 0 : rows * cols * 32, grid = fr_lsss_shares_grid(g, k);
    CheckedLds lds((size_t)FR_SHARES_CAP * NL + FR_LSSS_SHARES_WAVE);
    uint32_t active = 0;
    for (size_t block = 0; block < grid; block++) {
        lds.reset();
        if (!mat_step)
            for (uint32_t lane = 0; lane < FR_LSSS_SHARES_WAVE; lane++) fr_lsss_shares_stage(g, (uint32_t)block, lane, matrix, [&](uint32_t off, const Fr &v) { lds.put(off, v); });
        for (uint32_t lane = 0; lane < FR_LSSS_SHARES_WAVE && !lds.bad; lane++) {
            const LsssSharesLane l = fr_lsss_shares_map(g, (uint32_t)block, lane, k);
            if (!l.active) continue;
            if (l.item >= k || l.x >= rows) return -2;
            active++;
            const uint8_t *vec = vectors + l.item * cols * 32, *row = matrix + l.item * mat_step + (size_t)l.x * cols * 32;
            uint8_t *o = out + (l.item * rows + l.x) * 32;
            if (mat_step) fr_lsss_shares_lane([&](uint32_t c) { return fr_load_raw(row + 32 * (size_t)c); }, g.cols, vec, o);
            else fr_lsss_shares_lane([&](uint32_t c) { return lds.get(l.xr * g.pitch + c * NL); }, g.cols, vec, o);
        }
        if (lds.bad) return -2;
    }
    if (geom_out) { geom_out[0] = g.rg; geom_out[1] = g.nrg; geom_out[2] = g.ipb; geom_out[3] = g.pitch; geom_out[4] = (uint32_t)grid; geom_out[5] = active; }
    stats_flush();
    return 0;
}
// The LDS block of k_fr_find_common: set elements of eight words and single words (pos, keep) side by side.  A store outside the block, an
// element over anything stored before, a word inside an element, a load of an element's word through anything but the element's own
// offset and a load of a word that was not stored are refused.
struct CheckedWords {
    std::vector<uint32_t> w;
    std::vector<int64_t> owner;                 // -1 free, off: a word of the element at off, -2 - off: the single word at off
    bool bad = false;
    explicit CheckedWords(size_t words) : w(words, 0), owner(words, -1) {}
    void reset() { std::fill(owner.begin(), owner.end(), -1); }
    uint32_t gete(uint32_t off, int i) {
        if ((size_t)off + FR_SELECT_EW > w.size() || i < 0 || i >= FR_SELECT_EW || owner[off + i] != (int64_t)off) { bad = true; return 0; }
        return w[off + i];
    }
    void pute(uint32_t off, const uint32_t (&x)[FR_SELECT_EW]) {
        if ((size_t)off + FR_SELECT_EW > w.size()) { bad = true; return; }
        for (int i = 0; i < FR_SELECT_EW; i++) { if (owner[off + i] != -1) bad = true; owner[off + i] = off; w[off + i] = x[i]; }
    }
    uint32_t getw(uint32_t off) {
        if ((size_t)off >= w.size() || owner[off] != -2 - (int64_t)off) { bad = true; return 0; }
        return w[off];
    }
    void putw(uint32_t off, uint32_t x) {
        if ((size_t)off >= w.size() || (owner[off] != -1 && owner[off] != -2 - (int64_t)off)) { bad = true; return; }
        owner[off] = -2 - (int64_t)off;
        w[off] = x;
    }
};
// k_fr_find_common as it is launched: the geometry, the staging and the three phases behind it of select29.hip.hpp, workgroup by workgroup,
// a barrier = the end of a loop over the lanes.  geom_out: [lpi, ipb, chunks, pitch, large, shared, workgroups, active lanes].
// -1: arguments the entry refuses; -2: a refusal of the LDS stand-in, a lane outside the outputs, or a slot written twice or never.
int hc_fr_find_common(const uint8_t *sets, size_t n_sets, size_t m, const uint8_t *lists, size_t a, size_t d, size_t k, uint32_t *set_pos_out, uint32_t *list_pos_out,
                      uint8_t *common_out, uint8_t *ok_out, uint32_t *geom_out) {
    const size_t lim = (size_t)FR_SELECT_MAX;
    if (m < 1 || m > lim || a < 1 || a > lim || d < 1 || d > lim || !k || (n_sets != 1 && n_sets != k)) return -1;
    if (!sets || !lists || !set_pos_out || !list_pos_out || !common_out || !ok_out) return -1;
    const SelectGeom g = fr_select_geometry(m, a, d, n_sets == 1);
    CheckedWords lds((size_t)fr_select_words(g.large));
    const size_t grid = fr_select_grid(g, k);
    std::vector<uint8_t> slot_seen(k * d, 0), item_seen(k, 0);
    bool outside = false;
    uint32_t active = 0;
    const SelectOut o{(uint8_t *)set_pos_out, (uint8_t *)list_pos_out, common_out, ok_out, d * sizeof(uint32_t), d * 32};
    const auto gete = [&](uint32_t off, int i) { return lds.gete(off, i); };
    const auto getw = [&](uint32_t off) { return lds.getw(off); };
    const auto putw = [&](uint32_t off, uint32_t v) { lds.putw(off, v); };
    for (size_t block = 0; block < grid; block++) {
        lds.reset();
        for (uint32_t lane = 0; lane < FR_SELECT_WAVE; lane++)
            fr_select_stage(g, (uint32_t)block, lane, k, sets, [&](uint32_t off, const uint32_t (&w)[FR_SELECT_EW]) { lds.pute(off, w); });
        for (uint32_t lane = 0; lane < FR_SELECT_WAVE; lane++) {
            const SelectLane l = fr_select_map(g, (uint32_t)block, lane, k);
            if (l.active && l.item >= k) return -2;
            active += l.active ? 1u : 0u;
            fr_select_match(g, (uint32_t)block, lane, k, lists, gete, putw);
        }
        for (uint32_t lane = 0; lane < FR_SELECT_WAVE && !lds.bad; lane++) fr_select_mark(g, (uint32_t)block, lane, k, getw, putw);
        for (uint32_t lane = 0; lane < FR_SELECT_WAVE && !lds.bad; lane++)
            fr_select_pick(g, (uint32_t)block, lane, k, gete, getw,
                           [&](size_t item, uint32_t slot, uint32_t sp, uint32_t lp, const uint32_t (&w)[FR_SELECT_EW]) {
                               if (item >= k || slot >= d || slot_seen[item * d + slot]++) { outside = true; return; }
                               fr_select_store(o, item, slot, sp, lp, w);
                           },
                           [&](size_t item, bool ok) {
                               if (item >= k || item_seen[item]++) { outside = true; return; }
                               ok_out[item] = ok ? 1 : 0;
                           });
        if (lds.bad || outside) return -2;
    }
    if (std::count(slot_seen.begin(), slot_seen.end(), 1) != (ptrdiff_t)(k * d) || std::count(item_seen.begin(), item_seen.end(), 1) != (ptrdiff_t)k) return -2;
    if (geom_out) { geom_out[0] = g.lpi; geom_out[1] = g.ipb; geom_out[2] = g.chunks; geom_out[3] = g.pitch; geom_out[4] = g.large; geom_out[5] = g.shared; geom_out[6] = (uint32_t)grid; geom_out[7] = active; }
    stats_flush();
    return 0;
}
// k_fr_lsss_from_formula as it is launched: the staging, the walk and the write-out of formula29.hip.hpp, workgroup by workgroup, a barrier =
// the end of a loop over the lanes, the LDS block a CheckedWords of single words.  wide: the 128-bit store of a piece (matrix_out 16-byte
// aligned) or the byte stores.  geom_out: [items per workgroup, LDS words, workgroups, pieces written].
// -1: arguments the entry refuses; -2: a refusal of the LDS stand-in, a lane outside the outputs, or a piece, a rho or a verdict written twice or never.
int hc_fr_lsss_from_formula(const int64_t *nodes, size_t n_nodes, size_t k, size_t rows, size_t cols, uint8_t *matrix_out, int64_t *rho_out, uint32_t *dims_out, uint8_t *ok_out,
                            int wide, uint32_t *geom_out) {
    if (n_nodes < 1 || n_nodes > (size_t)FORMULA_MAX_NODES || rows < 1 || rows > (size_t)FORMULA_MAX || cols < 1 || cols > (size_t)FORMULA_MAX || !k) return -1;
    if (!nodes || !matrix_out || !rho_out || !ok_out || (wide && ((uintptr_t)matrix_out & 15))) return -1;
    const FormulaGeom g = formula_build_geometry(n_nodes, rows, cols, wide != 0);
    const FormulaOut o{matrix_out, (uint8_t *)rho_out, (uint8_t *)dims_out, ok_out, rows * cols * 32, rows * sizeof(int64_t), 2 * sizeof(uint32_t)};
    CheckedWords lds((size_t)FORMULA_BUILD_WORDS);
    const size_t grid = formula_grid(g, k), pieces = rows * cols * 2;
    std::vector<uint8_t> piece_seen(k * pieces, 0), rho_seen(k * rows, 0), item_seen(k, 0);
    bool outside = false;
    const auto getw = [&](uint32_t off) { return lds.getw(off); };
    const auto putw = [&](uint32_t off, uint32_t v) { lds.putw(off, v); };
    for (size_t block = 0; block < grid; block++) {
        lds.reset();
        for (uint32_t lane = 0; lane < FORMULA_WAVE; lane++) formula_stage(g, (uint32_t)block, lane, k, nodes, putw);
        for (uint32_t lane = 0; lane < FORMULA_WAVE && !lds.bad; lane++) formula_build_walk(g, (uint32_t)block, lane, k, getw, putw);
        for (uint32_t lane = 0; lane < FORMULA_WAVE && !lds.bad; lane++)
            formula_build_write(g, (uint32_t)block, lane, k, getw,
                                [&](size_t item, uint32_t p, const uint32_t (&w)[4]) {
                                    if (item >= k || p >= pieces || piece_seen[item * pieces + p]++) { outside = true; return; }
                                    formula_store_piece(g, o, item, p, w);
                                },
                                [&](size_t item, uint32_t x, int64_t a) {
                                    if (item >= k || x >= rows || rho_seen[item * rows + x]++) { outside = true; return; }
                                    formula_store_rho(o, item, x, a);
                                },
                                [&](size_t item, bool ok, uint32_t nrows, uint32_t ncols) {
                                    if (item >= k || item_seen[item]++) { outside = true; return; }
                                    formula_store_done(o, item, ok, nrows, ncols);
                                });
        if (lds.bad || outside) return -2;
    }
    if (std::count(piece_seen.begin(), piece_seen.end(), 1) != (ptrdiff_t)(k * pieces) || std::count(rho_seen.begin(), rho_seen.end(), 1) != (ptrdiff_t)(k * rows) ||
        std::count(item_seen.begin(), item_seen.end(), 1) != (ptrdiff_t)k)
        return -2;
    if (geom_out) { geom_out[0] = g.ipb; geom_out[1] = (uint32_t)FORMULA_BUILD_WORDS; geom_out[2] = (uint32_t)grid; geom_out[3] = (uint32_t)(k * pieces); }
    return 0;
}
// k_formula_select as it is launched.  geom_out: [items per workgroup, pitch, shared, workgroups].  Return codes as above.
int hc_formula_select(const int64_t *nodes, size_t n_formulas, size_t n_nodes, const uint8_t *held, size_t k, size_t rows, uint8_t *chosen_out, uint8_t *ok_out, uint32_t *geom_out) {
    if (n_nodes < 1 || n_nodes > (size_t)FORMULA_MAX_NODES || rows < 1 || rows > (size_t)FORMULA_MAX || !k || (n_formulas != 1 && n_formulas != k)) return -1;
    if (!nodes || !held || !chosen_out || !ok_out) return -1;
    const FormulaGeom g = formula_select_geometry(n_nodes, rows, n_formulas == 1 && k > 1);
    CheckedWords lds((size_t)FORMULA_SELECT_WORDS);
    const size_t grid = formula_grid(g, k);
    std::vector<uint8_t> item_seen(k, 0);
    bool outside = false;
    for (size_t block = 0; block < grid; block++) {
        lds.reset();
        for (uint32_t lane = 0; lane < FORMULA_WAVE; lane++) formula_stage(g, (uint32_t)block, lane, k, nodes, [&](uint32_t off, uint32_t v) { lds.putw(off, v); });
        for (uint32_t lane = 0; lane < FORMULA_WAVE && !lds.bad; lane++)
            formula_select_lane(g, (uint32_t)block, lane, k, [&](uint32_t off) { return lds.getw(off); }, held,
                                [&](size_t item, bool ok, uint64_t chosen) {
                                    if (item >= k || item_seen[item]++) { outside = true; return; }
                                    formula_store_chosen(g, chosen_out, ok_out, item, ok, chosen);
                                });
        if (lds.bad || outside) return -2;
    }
    if (std::count(item_seen.begin(), item_seen.end(), 1) != (ptrdiff_t)k) return -2;
    if (geom_out) { geom_out[0] = g.ipb; geom_out[1] = g.pitch; geom_out[2] = g.shared; geom_out[3] = (uint32_t)grid; }
    return 0;
}
// The seed-addressed generator (csrc/chacha29.hip.hpp, fr_wide_reduce of csrc/fr29.hip.hpp) as the kernels of csrc/gpbc_hash.hip run a
// lane.  hc_chacha_blocks is k_random_bytes: the key from the seed bytes, index first + i by a 64-bit add, the block, its 64 bytes through
// the 128-bit or the byte stores.  hc_fr_wide_reduce is k_fr_set_bytes64: sixteen words in, the reduction under the interval bounds (the
// product's columns, the canonical form's range), 32 bytes out.  hc_fr_random is k_fr_random: the two in a row.
int hc_chacha_blocks(const uint8_t *seed, uint64_t stream, uint64_t first, size_t n, uint8_t *out, int wide) {
    if (!seed || !out || (first && n > (size_t)0 - first) || (wide && ((uintptr_t)out & 15))) return -1;
    const ChaChaKey key = chacha_key(seed, stream);
    for (size_t i = 0; i < n; i++) {
        uint32_t w[16];
        chacha20_block(w, key, first + i);
        chacha_store<4>(out + 64 * i, w, wide != 0);
    }
    return 0;
}
int hc_fr_wide_reduce(const uint8_t *in, size_t n, uint8_t *out, int wide_in, int wide_out) {
    if (!in || !out || (wide_in && ((uintptr_t)in & 15)) || (wide_out && ((uintptr_t)out & 15))) return -1;
    for (size_t i = 0; i < n; i++) {
        uint32_t w[16], s[8];
        chacha_load64(w, in + 64 * i, wide_in != 0);
        fr_words(s, fr_wide_reduce(w));
        chacha_store<2>(out + 32 * i, s, wide_out != 0);
    }
    stats_flush();
    return 0;
}
int hc_fr_random(const uint8_t *seed, uint64_t stream, uint64_t first, size_t n, uint8_t *out) {
    if (!seed || !out || (first && n > (size_t)0 - first)) return -1;
    const ChaChaKey key = chacha_key(seed, stream);
    for (size_t i = 0; i < n; i++) {
        uint32_t w[16], s[8];
        chacha20_block(w, key, first + i);
        fr_words(s, fr_wide_reduce(w));
        chacha_store<2>(out + 32 * i, s, false);
    }
    stats_flush();
    return 0;
}
}  // extern "C"
// k_fr_dot_segments as gpbc_fr_dot_segments_dev runs it (csrc/gpbc_fr.hip): the plan and the level walk of csrc/segred29.hip.hpp with
// FR_DOT_SHAPE, fr_dot_lanes(g) lanes per piece and a wavefront of 64 lanes at a time — fr_dot_lane for each of them with the wavefront's
// trip count (piece slots past the last piece are empty pieces), the butterfly steps of the fold on all 64 values at once, fr_dot_store
// by the first lane of every piece.  levels_out: [the number of levels the plan took, the OR of the lanes-per-piece values of its
// launches].  -1: arguments the entry refuses.
#include "../gopairingbasedcryptography_amd/csrc/frdot29.hip.hpp"
extern "C" {
int hc_fr_dot_segments(const uint8_t *A, const uint8_t *B, size_t nb, const uint64_t *seg_off, size_t n, size_t n_seg, uint8_t *out, uint32_t *levels_out) {
    if (!n_seg || !seg_off || (n && !A) || !out || (!B && nb) || (B && nb != n && (nb > n || nb * n_seg != n))) return -1;
    const SegRedPlan plan = segred_plan(FR_DOT_SHAPE, 32, 0, n, n_seg, B != nullptr);
    std::vector<uint8_t> v0(plan.val_bytes[0]), v1(plan.val_bytes[1]);
    uint8_t *const val[2] = {v0.data(), v1.data()};
    uint32_t levels = 0, lanes_used = 0;
    segred_walk(FR_DOT_SHAPE, segred_args(A, B, nb, seg_off, n, n_seg), val, out, [&](SegRedArgs g, size_t pieces) {
        g.n_pieces = pieces;
        levels++;
        const uint32_t L = fr_dot_lanes(g), per_wave = FR_DOT_WAVE / L;
        lanes_used |= L;
        for (size_t w = 0; w < (pieces + per_wave - 1) / per_wave; w++) {
            size_t lo[FR_DOT_WAVE], a[FR_DOT_WAVE], b[FR_DOT_WAVE], P[FR_DOT_WAVE], rounds = 0;
            bool have[FR_DOT_WAVE];
            for (uint32_t t = 0; t < FR_DOT_WAVE; t++) {
                have[t] = segred_piece(g, w * per_wave + t / L, lo[t], a[t], b[t], P[t]);
                if (!have[t]) lo[t] = a[t] = b[t] = P[t] = 0;
                const size_t r = fr_dot_rounds(b[t] - a[t], L);
                rounds = r > rounds ? r : rounds;
            }
            Fr v[FR_DOT_WAVE];
            for (uint32_t t = 0; t < FR_DOT_WAVE; t++) v[t] = fr_dot_lane(g.x, g.k, g.k_shared ? lo[t] : 0, a[t], b[t], t % L, L, rounds, false, false);
            for (uint32_t off = L / 2; off >= 1; off >>= 1) {
                Fr nv[FR_DOT_WAVE];
                for (uint32_t t = 0; t < FR_DOT_WAVE; t++) nv[t] = fr_dot_fold(v[t], v[t ^ off]);
                for (uint32_t t = 0; t < FR_DOT_WAVE; t++) v[t] = nv[t];
            }
            for (uint32_t t = 0; t < FR_DOT_WAVE; t += L)
                if (have[t]) fr_dot_store(g.out + P[t] * 32, v[t]);
        }
        return 0;
    });
    if (levels_out) { levels_out[0] = levels; levels_out[1] = lanes_used; }
    stats_flush();
    return 0;
}
// the shape constants, for the tests' restatement of the plan: [fill, group, plain_min, lanes of a wavefront, FR_DOT_NORM, FR_DOT_RUN_MUL, FR_DOT_RUN_SUM, FR_DOT_LANES_MIN]
void hc_fr_dot_shape(uint32_t *o) {
    o[0] = (uint32_t)FR_DOT_SHAPE.fill; o[1] = (uint32_t)FR_DOT_SHAPE.group; o[2] = (uint32_t)FR_DOT_SHAPE.plain_min; o[3] = FR_DOT_WAVE;
    o[4] = FR_DOT_NORM; o[5] = FR_DOT_RUN_MUL; o[6] = FR_DOT_RUN_SUM; o[7] = FR_DOT_LANES_MIN;
}
}  // extern "C"
// k_g1_fb_indexed / k_g2_fb_indexed as they are launched: the window tables of the bases (only the rows the scalars reach are built, by
// the scalar multiplication k_g1/g2_fb_build uses), then fb_index_map / fb_index_output / fb_indexed_lane for every lane of every
// workgroup.  group_min: as GPBC_FBINDEX_GROUP_MIN of the build (0 = its default 64).  geom_out: [grouped, workgroups, lanes with an
// output].  -1: arguments the entry refuses; -2: a lane outside the outputs or an output owned twice.
template <class F, class LoadA, class StoreA> static int fb_indexed_host(const uint8_t *B, size_t nbase, const uint32_t *index, size_t n_index_rows, size_t terms, const uint8_t *K, size_t n,
                                                                          size_t group_min, uint8_t *out, uint8_t *ok_out, uint32_t *geom_out, size_t pt, LoadA ld, StoreA st) {
    constexpr size_t ED = (size_t)TabLayout<F>::ENTRY_DWORDS;
    std::vector<int32_t> mem(nbase * (size_t)FBI_ENTRIES * ED + 32);
    int32_t *table = mem.data();
    while ((uintptr_t)table & 127) table++;                // rows 128-byte aligned like the device's
    std::vector<uint8_t> inf(nbase), built(nbase * (size_t)FBI_ENTRIES, 0);
    std::vector<AffP<F>> bases(nbase);
    for (size_t b = 0; b < nbase; b++) { bases[b] = ld(B + pt * b); inf[b] = bases[b].inf ? 1 : 0; }
    for (size_t i = 0; i < n; i++)
        for (size_t t = 0; t < terms; t++) {
            const uint32_t j = index[(i % n_index_rows) * terms + t];
            if (j == FBI_NONE || j >= nbase || inf[j]) continue;
            uint32_t k[8]; memcpy(k, K + 32 * (i * terms + t), 32);
            for (int w = 0; w < FBI_WINDOWS; w++) {
                const int d = (int)((k[w >> 2] >> (8 * (w & 3))) & 255u);
                const size_t e = ((size_t)j * FBI_WINDOWS + w) * FBI_DIGITS + d - 1;
                if (!d || built[e]) continue;
                uint32_t kk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                kk[w >> 2] = (uint32_t)d << (8 * (w & 3));
                alignas(16) int32_t tab[glv_table_dwords<F>()];
                JacP<F> r; scalar_mul29_best(r, bases[j], kk, tab);
                AffP<F> a; jac_to_affine(a, r);
                tab_store(table + e * ED, 0, a);
                built[e] = 1;
            }
        }
    const FbIndexMap map = fb_index_map(n, n_index_rows, group_min ? group_min : 64);
    const size_t grid = fb_index_grid(map);
    std::vector<uint8_t> seen(n, 0);
    uint32_t lanes = 0;
    for (size_t block = 0; block < grid; block++)
        for (uint32_t lane = 0; lane < FBI_WAVE; lane++) {
            const size_t i = fb_index_output(map, block, lane);
            if (i == n) continue;
            if (i > n || seen[i]) return -2;
            seen[i] = 1; lanes++;
            fb_indexed_lane<F>(table, inf.data(), nbase, index + (i % map.P) * terms, (uint32_t)terms, K + 32 * i * terms, out + pt * i, ok_out ? ok_out + i : nullptr,
                               [](uint32_t *k, const uint8_t *p) { memcpy(k, p, 32); }, st);
        }
    if (geom_out) { geom_out[0] = map.grouped; geom_out[1] = (uint32_t)grid; geom_out[2] = lanes; }
    return lanes == n ? 0 : -2;
}
extern "C" {
int hc_fb_indexed(int is_g2, const uint8_t *B, size_t nbase, const uint32_t *index, size_t n_index_rows, size_t terms, const uint8_t *K, size_t n, size_t group_min, uint8_t *out,
                  uint8_t *ok_out, uint32_t *geom_out) {
    if (terms < 1 || terms > FBI_MAX_TERMS || !n || n_index_rows < 1 || n_index_rows > n || !nbase || !B || !index || !K || !out) return -1;
    int rc;
    if (is_g2)
        rc = fb_indexed_host<F2>(B, nbase, index, n_index_rows, terms, K, n, group_min, out, ok_out, geom_out, 128,
                                 [](const uint8_t *p) { return AffP<F2>{f2_load(p), f2_load(p + 64), bytes_all_zero(p, 32)}; },
                                 [](uint8_t *p, const AffP<F2> &r) { f2_store(p, r.x); f2_store(p + 64, r.y); });
    else
        rc = fb_indexed_host<Fe>(B, nbase, index, n_index_rows, terms, K, n, group_min, out, ok_out, geom_out, 64,
                                 [](const uint8_t *p) { return AffP<Fe>{fe_load(p), fe_load(p + 32), bytes_all_zero(p, 16)}; },
                                 [](uint8_t *p, const AffP<Fe> &r) { fe_store(p, r.x); fe_store(p + 32, r.y); });
    stats_flush();
    return rc;
}
// worst-case figures since process start: [max |int64 column|, max limb bound, max value bound (units of p),
// #products (fe_mul + fe_mul2), #norms, #fe_mul2, #reduces]  (out must hold 7 doubles)
// v_mad_i64_i32 the device form of everything run since the last call would have executed (summed over the lanes of a pair)
double hc_mads_take(void) {
    stats_flush();
    std::lock_guard<std::mutex> lk(g_stats_mu);
    const double m = (double)g_stats_total.mads;
    g_stats_total.mads = 0;
    return m;
}
void hc_stats(double *out) {
    stats_flush();
    BoundStats &s = g_stats_total;
    out[0] = s.max_col; out[1] = s.max_limb; out[2] = s.max_vb; out[3] = (double)s.muls; out[4] = (double)s.norms; out[5] = (double)s.muls2; out[6] = (double)s.reduces;
}
}

// ------------------------------------------------------------------------------------------------ threshold-tree forests
#include "../gopairingbasedcryptography_amd/csrc/forest29.hip.hpp"
extern "C" {
// the plan of a forest alone: sizes_out [T, Lmax, Gmax, Cmax, Umax, depth_max, narrowest level, widest level, Emax, Pmax]; -1, the tree the
// reason belongs to in *bad_tree (T: the forest itself) and the reason in why (up to 96 bytes) when it is refused
int hc_fr_forest_plan(const uint32_t *nodes, const uint32_t *node_off, size_t n_trees, uint32_t *sizes_out, size_t *bad_tree, char *why) {
    ForestPlan f;
    size_t bad = 0;
    const char *w = fr_forest_plan(reinterpret_cast<const ShareNode *>(nodes), node_off, n_trees, f, &bad);
    if (bad_tree) *bad_tree = bad;
    if (w) { if (why) snprintf(why, 96, "%s", w); return -1; }
    if (!fr_forest_plan_ok(f)) return -2;
    if (sizes_out) {
        const uint32_t v[10] = {f.T, f.Lmax, f.Gmax, f.Cmax, f.Umax, f.depth_max, f.wmin, f.wmax, f.Emax, f.Pmax};
        memcpy(sizes_out, v, sizeof(v));
    }
    return 0;
}
// k_fr_share_forest as it is launched: the plan, the block check, the geometry, the item mapping, the staging, every level to the forest's
// depth and the finish of forest29.hip.hpp, workgroup by workgroup, a barrier = the end of a loop over the lanes.
// geom_out: [Lmax, Cmax, depth, ipb, lpi, pitch, large, workgroups].  -1: a refused forest or argument; -2: a refusal of the LDS stand-in
// or a block that fails its check.
int hc_fr_share_forest(const uint32_t *nodes, const uint32_t *node_off, size_t n_trees, const uint32_t *tree_of, const uint8_t *secrets, const uint8_t *coeffs, size_t k, uint8_t *out,
                       uint8_t *ok_out, uint32_t *geom_out) {
    ForestPlan f;
    size_t bad = 0;
    if (fr_forest_plan(reinterpret_cast<const ShareNode *>(nodes), node_off, n_trees, f, &bad) || !k || !tree_of || !secrets || !out || (f.Cmax && !coeffs)) return -1;
    if (!fr_forest_plan_ok(f)) return -2;
    const ForestGeom g = fr_forest_share_geometry(f);
    const size_t cap = (size_t)(g.large ? FR_TREE_LARGE : FR_TREE_SMALL) * NL + FR_SHARE_WAVE;
    if (g.ipb * g.lpi != (uint32_t)FR_SHARE_WAVE || (size_t)g.ipb * g.pitch > cap) return -2;
    const ForestDev fd{f.trees.data(), f.sunits.data(), f.runits.data(), f.level_off.data(), f.gate_off.data(), f.gates.data()};
    CheckedLds lds(cap);
    const size_t grid = fr_forest_grid(g, k);
    const auto get = [&](uint32_t off) { return lds.get(off); };
    const auto put = [&](uint32_t off, const Fr &v) { lds.put(off, v); };
    std::vector<ForestItem> its(FR_SHARE_WAVE);
    for (size_t block = 0; block < grid; block++) {
        lds.reset();
        for (uint32_t lane = 0; lane < FR_SHARE_WAVE; lane++) {
            its[lane] = fr_forest_item(g, fd.trees, tree_of, (uint32_t)block, lane, k);
            fr_forest_share_stage(g, its[lane], secrets, coeffs, put);
        }
        for (uint32_t lv = 1; lv <= g.depth && !lds.bad; lv++)
            for (uint32_t lane = 0; lane < FR_SHARE_WAVE; lane++) fr_forest_share_level(g, its[lane], fd, lv, get, put, out);
        for (uint32_t lane = 0; lane < FR_SHARE_WAVE; lane++) fr_forest_share_finish(g, its[lane], secrets, out, ok_out);
        if (lds.bad) return -2;
    }
    if (geom_out) { const uint32_t v[8] = {g.Lmax, g.Cmax, g.depth, g.ipb, g.lpi, g.pitch, g.large, (uint32_t)grid}; memcpy(geom_out, v, sizeof(v)); }
    stats_flush();
    return 0;
}
// k_fr_forest_weights as it is launched, in the same way: staging, UP and DOWN to the forest's depth, the finish.  geom_out as above.
int hc_fr_forest_weights(const uint32_t *nodes, const uint32_t *node_off, size_t n_trees, const uint32_t *tree_of, const uint8_t *held, size_t k, uint8_t *w_out, uint8_t *ok_out,
                         uint32_t *geom_out) {
    ForestPlan f;
    size_t bad = 0;
    if (fr_forest_plan(reinterpret_cast<const ShareNode *>(nodes), node_off, n_trees, f, &bad) || !k || !tree_of || !held || !w_out || !ok_out) return -1;
    if (!fr_forest_plan_ok(f)) return -2;
    const ForestGeom g = fr_forest_recon_geometry(f);
    const size_t cap = (size_t)(g.large ? FR_RECON_LARGE : FR_RECON_SMALL);
    if (g.ipb * g.lpi != (uint32_t)FR_RECON_WAVE || (size_t)g.ipb * g.pitch > cap) return -2;
    const ForestDev fd{f.trees.data(), f.sunits.data(), f.runits.data(), f.level_off.data(), f.gate_off.data(), f.gates.data()};
    CheckedLds lds(cap + FR_RECON_WAVE);
    const size_t grid = fr_forest_grid(g, k);
    const auto get = [&](uint32_t off) { return lds.get(off); };
    const auto put = [&](uint32_t off, const Fr &v) { lds.put(off, v); };
    const auto getw = [&](uint32_t off) { return lds.getw(off); };
    const auto putw = [&](uint32_t off, uint32_t v) { lds.putw(off, v); };
    std::vector<ForestItem> its(FR_RECON_WAVE);
    for (size_t block = 0; block < grid; block++) {
        lds.reset();
        for (uint32_t lane = 0; lane < FR_RECON_WAVE; lane++) {
            its[lane] = fr_forest_item(g, fd.trees, tree_of, (uint32_t)block, lane, k);
            fr_forest_recon_stage(g, its[lane], fd, held, put, putw);
        }
        for (uint32_t lv = g.depth; lv-- > 0 && !lds.bad;)
            for (uint32_t lane = 0; lane < FR_RECON_WAVE; lane++) fr_forest_recon_up(g, its[lane], fd, lv, getw, putw, ok_out);
        for (uint32_t lv = 1; lv <= g.depth && !lds.bad; lv++)
            for (uint32_t lane = 0; lane < FR_RECON_WAVE; lane++) fr_forest_recon_down<FR_RECON_G>(g, its[lane], fd, lv, get, put, getw, putw, w_out);
        for (uint32_t lane = 0; lane < FR_RECON_WAVE; lane++) fr_forest_recon_finish(g, its[lane], held, w_out, ok_out);
        if (lds.bad) return -2;
    }
    if (geom_out) { const uint32_t v[8] = {g.Lmax, g.Cmax, g.depth, g.ipb, g.lpi, g.pitch, g.large, (uint32_t)grid}; memcpy(geom_out, v, sizeof(v)); }
    stats_flush();
    return 0;
}
}

// ------------------------------------------------------------------------------------------------ membership of in-memory elements
#include "../gopairingbasedcryptography_amd/csrc/member29.hip.hpp"
extern "C" {
// the lane bodies of k_g1_is_on_curve, k_g2_is_on_curve (curve_only = 1) / k_g2_is_in_subgroup and k_gt_is_in_subgroup, a verdict byte per
// element.  force = 1 runs every GT element through the whole chain, whatever the earlier tests said: what a lane pair does on the device
// beside a neighbour that is still a candidate — the limb-bound proof for non-cyclotomic values in the Granger-Scott squarings; force = 0
// is the wavefront skip with the pair as the whole wavefront.
void hc_g1_is_on_curve(const uint8_t *P, size_t n, uint8_t *ok) {
    for (size_t i = 0; i < n; i++) ok[i] = g1_member_on_curve(P + 64 * i) ? 1 : 0;
    stats_flush();
}
void hc_g2_is_in_subgroup(const uint8_t *P, size_t n, uint8_t *ok, int curve_only) {
    for (size_t i = 0; i < n; i++) ok[i] = g2_member(P + 128 * i, !curve_only) ? 1 : 0;
    stats_flush();
}
void hc_gt_is_in_subgroup(const uint8_t *Z, size_t n, uint8_t *ok, int force) {
    for (size_t i = 0; i < n; i++) {
        PairRendezvous rv;
        bool verdict[2];
        auto lane = [&](bool odd) {
            PairHost x{odd, &rv};
            verdict[odd] = gt_member_pair(x, Z + 384 * i + (odd ? 192 : 0), force != 0);
            stats_flush();
        };
        std::thread t1(lane, true);
        lane(false);
        t1.join();
        ok[i] = verdict[0] ? (verdict[1] ? 1 : 2) : (verdict[1] ? 2 : 0);      // 2: the two lanes of a pair disagree (never)
    }
}
}

// ------------------------------------------------------------------------------------------------ fixed-base exponentiation in GT
#include "../gopairingbasedcryptography_amd/csrc/gtfixed29.hip.hpp"
// jobs 0 .. n_jobs - 1, each a lane pair on two threads of its own, a few pairs side by side (the pairs share nothing but the statistics)
template <class Job> static void gt_fb_pairs(size_t n_jobs, Job job) {
    const size_t width = std::max<size_t>(1, std::min<size_t>(16, std::thread::hardware_concurrency() / 2));
    for (size_t lo = 0; lo < n_jobs; lo += width) {
        std::vector<PairRendezvous> rv(std::min(width, n_jobs - lo));
        std::vector<std::thread> th;
        for (size_t q = 0; q < rv.size(); q++)
            for (int odd = 0; odd < 2; odd++)
                th.emplace_back([&, q, odd] { job(PairHost{odd != 0, &rv[q]}, lo + q); stats_flush(); });
        for (auto &t : th) t.join();
    }
}
extern "C" {
// the lane bodies of k_gt_fb_build and k_gt_fb_indexed (csrc/gpbc_gtfixed.hip) with the kernels' own addressing: table = nbase x 4 MiB of
// int32 (gpbc_gt_fixed_base_table_bytes), one lane pair per (base, window) and per output.  In the build the pair is the wavefront, so
// w_max is its own window.  -1: arguments the entry refuses.
int hc_gt_fb_build(const uint8_t *B, size_t nbase, int32_t *table) {
    if (!B || !nbase || !table) return -1;
    gt_fb_pairs(nbase * GTFB_WINDOWS, [&](const PairHost &x, size_t q) {
        const size_t j = q / GTFB_WINDOWS;
        const int w = (int)(q % GTFB_WINDOWS);
        gt_fb_build_lane(x, B + 384 * j + (x.odd ? 192 : 0), w, w, table + j * GTFB_BASE_DWORDS + (size_t)w * GTFB_WINDOW_DWORDS);
    });
    return 0;
}
int hc_gt_fb_indexed(const int32_t *table, size_t nbase, const uint32_t *index, size_t n_index_rows, size_t terms, const uint8_t *K, size_t n, uint8_t *out, uint8_t *ok_out) {
    if (!table || !nbase || terms < 1 || terms > FBI_MAX_TERMS || n > (size_t)0xffffffffu / terms) return -1;
    if (!n) return 0;
    if (n_index_rows < 1 || n_index_rows > n || !index || !K || !out) return -1;
    gt_fb_pairs(n, [&](const PairHost &x, size_t i) {
        gt_fb_indexed_lane(x, table, nbase, index + (i % n_index_rows) * terms, (uint32_t)terms, K + 32 * i * terms, out + 384 * i + (x.odd ? 192 : 0), ok_out ? ok_out + i : nullptr,
                           [](uint32_t *k, const uint8_t *p) { memcpy(k, p, 32); });
    });
    return 0;
}
}

// ------------------------------------------------------------------------------------------------ opening proofs over ragged batches
#include "../gopairingbasedcryptography_amd/csrc/openings29.hip.hpp"
// k_g1/g2_fb_openings as gpbc_fixed_base_openings_dev launches them: the blocks of the segment table (opn_blocks), one lane per (identity,
// chunk of C bases) through fb_openings_lane with f's coefficients canonical as the staging leaves them, the partial sums chunk-major, then
// the fan-in-16 levels of the strided point sum and the mask.  The window tables hold the rows the quotients reach (found by a first walk
// of the same steps) and are kept from call to call while the bases stay the same.
template <class F> struct OpnTables {
    std::vector<uint8_t> bases;
    std::vector<int32_t> mem;
    std::vector<uint8_t> built;
    int32_t *table = nullptr;
};
template <class F, class LoadA, class StoreA> static int fb_openings_host(const uint8_t *B, size_t nbase, const uint8_t *coeffs, const uint8_t *ids, const uint64_t *seg_off, size_t k, size_t C,
                                                                          uint8_t *out, uint8_t *ok_out, size_t pt, LoadA ld, StoreA st) {
    constexpr size_t ED = (size_t)TabLayout<F>::ENTRY_DWORDS;
    static OpnTables<F> T;
    if (T.bases.size() != nbase * pt || memcmp(T.bases.data(), B, nbase * pt)) {
        T.bases.assign(B, B + nbase * pt);
        T.mem.assign(nbase * (size_t)OPN_ENTRIES * ED + 32, 0);
        T.built.assign(nbase * (size_t)OPN_ENTRIES, 0);
        T.table = T.mem.data();
        while ((uintptr_t)T.table & 127) T.table++;                // rows 128-byte aligned like the device's
    }
    std::vector<uint8_t> inf(nbase);
    std::vector<AffP<F>> bases(nbase);
    for (size_t b = 0; b < nbase; b++) { bases[b] = ld(B + pt * b); inf[b] = bases[b].inf ? 1 : 0; }
    const size_t n = (size_t)seg_off[k], n_blocks = opn_blocks(seg_off, k, nullptr), n_chunks = (nbase + C - 1) / C;
    std::vector<OpnBlock> blocks(n_blocks);
    opn_blocks(seg_off, k, blocks.data());
    std::vector<Fr> cs(nbase);
    for (const OpnBlock &b : blocks) {                             // the rows the quotients of this block reach
        for (uint32_t i = 0; i <= b.m; i++) cs[i] = fr_poly_coeff_in(coeffs + ((size_t)b.seg * nbase + i) * 32);
        for (uint32_t lane = 0; lane < b.rows; lane++) {
            const Fr point = fr_poly_point(ids + 32 * ((size_t)b.id0 + lane));
            Fr carry = fr_zero();
            for (uint32_t c = b.m; c-- > 0;) {
                carry = fr_poly_horner_step(carry, cs[c + 1], point);
                if (inf[c]) continue;
                uint32_t kw[8]; fr_words(kw, carry);
                for (int w = 0; w < OPN_WINDOWS; w++) {
                    const int d = (int)((kw[w >> 2] >> (8 * (w & 3))) & 255u);
                    const size_t e = ((size_t)c * OPN_WINDOWS + w) * OPN_DIGITS + d - 1;
                    if (!d || T.built[e]) continue;
                    uint32_t kk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    kk[w >> 2] = (uint32_t)d << (8 * (w & 3));
                    alignas(16) int32_t tab[glv_table_dwords<F>()];
                    JacP<F> r; scalar_mul29_best(r, bases[c], kk, tab);
                    AffP<F> a; jac_to_affine(a, r);
                    tab_store(T.table + e * ED, 0, a);
                    T.built[e] = 1;
                }
            }
        }
    }
    std::vector<uint8_t> partial(n_chunks * n * pt + 64, 0xC3), flags(n + 16, 0xC3);
    std::vector<uint8_t> seen(n_chunks * n, 0);
    for (size_t wg = 0; wg < n_blocks * n_chunks; wg++) {          // the grid, chunk-major
        const uint32_t chunk = (uint32_t)(wg / n_blocks);
        const OpnBlock &b = blocks[wg % n_blocks];
        const uint32_t c_lo = chunk * (uint32_t)C, c_hi = (size_t)c_lo + C < nbase ? c_lo + (uint32_t)C : (uint32_t)nbase;
        if (c_lo < b.m)
            for (uint32_t i = 0; i <= b.m; i++) cs[i] = fr_poly_coeff_in(coeffs + ((size_t)b.seg * nbase + i) * 32);
        for (uint32_t lane = 0; lane < b.rows; lane++) {
            const size_t i = (size_t)b.id0 + lane, slot = (size_t)chunk * n + i;
            if (i >= n || seen[slot]) return -2;
            seen[slot] = 1;
            fb_openings_lane<F>(T.table, inf.data(), [&](uint32_t c) { return cs[c]; }, b.m, ids + 32 * i, c_lo, c_hi, C >= nbase, partial.data() + slot * pt, flags.data() + i, st);
        }
    }
    for (size_t s = 0; s < n_chunks * n; s++) if (!seen[s]) return -2;
    for (size_t g = n_chunks * n * pt; g < partial.size(); g++) if (partial[g] != 0xC3) return -3;
    for (size_t g = n; g < flags.size(); g++) if (flags[g] != 0xC3) return -3;
    std::vector<uint8_t> level;
    for (size_t c = n_chunks; c > 1;) {                            // k_g1/g2_sum_level: out[t] = in[t] + in[t + n_out] + ...
        const size_t c2 = (c + 15) / 16, n_in = c * n, n_out = c2 * n;
        level.assign(n_out * pt, 0);
        for (size_t t = 0; t < n_out; t++) {
            JacP<F> acc; jac_set_inf(acc);
            for (size_t i = t; i < n_in; i += n_out) jac_add_mixed(acc, acc, ld(partial.data() + i * pt));
            AffP<F> r; jac_to_affine(r, acc);
            st(level.data() + t * pt, r);
        }
        partial.swap(level); c = c2;
    }
    for (size_t i = 0; i < n; i++) {
        if (n_chunks > 1 && !flags[i]) memset(out + i * pt, 0, pt); else memcpy(out + i * pt, partial.data() + i * pt, pt);
        if (ok_out) ok_out[i] = flags[i];
    }
    return 0;
}
extern "C" {
// -1: arguments the entries refuse.  k_fr_poly_from_roots_segments: the steps of hc_fr_poly_from_roots per segment, rows of `stride` scalars
int hc_fr_poly_from_roots_segments(const uint8_t *roots, const uint64_t *seg_off, size_t k, size_t stride, uint8_t *coeffs_out) {
    if (!seg_off || seg_off[0] != 0 || stride < 1 || stride > ((size_t)1 << 24) || !coeffs_out) return -1;
    for (size_t j = 0; j < k; j++)
        if (seg_off[j + 1] < seg_off[j] || seg_off[j + 1] - seg_off[j] > (uint64_t)FR_POLY_MAX_B || seg_off[j + 1] - seg_off[j] + 1 > stride) return -1;
    if (seg_off[k] && !roots) return -1;
    std::vector<Fr> cs(FR_POLY_MAX_B + 1), nw(FR_POLY_MAX_B + 1);
    for (size_t j = 0; j < k; j++) {
        const size_t lo = (size_t)seg_off[j], B = (size_t)(seg_off[j + 1] - seg_off[j]);
        for (size_t i = 0; i <= B; i++) cs[i] = i ? fr_zero() : fr_plain_one();
        for (size_t s = 0; s < B; s++) {
            const Fr nr = fr_poly_neg_root(roots + (lo + s) * 32);
            for (size_t i = 0; i <= s + 1; i++) nw[i] = fr_poly_root_step(i ? cs[i - 1] : fr_zero(), cs[i], nr);
            for (size_t i = 0; i <= s + 1; i++) cs[i] = nw[i];
        }
        for (size_t i = 0; i <= B; i++) fr_poly_store(coeffs_out + (j * stride + i) * 32, cs[i]);
        memset(coeffs_out + (j * stride + B + 1) * 32, 0, (stride - B - 1) * 32);
    }
    stats_flush();
    return 0;
}
// C: bases per lane (the entry takes opn_shape's; here 1 .. nbase and beyond are walked); -2: a lane outside the grid's outputs or one
// owned twice; -3: a write outside the partial sums or the flags
int hc_fb_openings(int is_g2, const uint8_t *B, size_t nbase, const uint8_t *coeffs, const uint8_t *ids, const uint64_t *seg_off, size_t k, size_t C, uint8_t *out, uint8_t *ok_out) {
    if (!B || !nbase || !seg_off || seg_off[0] != 0 || C < 1) return -1;
    for (size_t j = 0; j < k; j++)
        if (seg_off[j + 1] < seg_off[j] || seg_off[j + 1] - seg_off[j] > (uint64_t)FR_POLY_MAX_B || seg_off[j + 1] - seg_off[j] + 1 > nbase) return -1;
    if (!k || !seg_off[k]) return 0;
    if (!coeffs || !ids || !out) return -1;
    int rc;
    if (is_g2)
        rc = fb_openings_host<F2>(B, nbase, coeffs, ids, seg_off, k, C, out, ok_out, 128,
                                  [](const uint8_t *p) { return AffP<F2>{f2_load(p), f2_load(p + 64), bytes_all_zero(p, 32)}; },
                                  [](uint8_t *p, const AffP<F2> &r) { f2_store(p, r.x); f2_store(p + 64, r.y); });
    else
        rc = fb_openings_host<Fe>(B, nbase, coeffs, ids, seg_off, k, C, out, ok_out, 64,
                                  [](const uint8_t *p) { return AffP<Fe>{fe_load(p), fe_load(p + 32), bytes_all_zero(p, 16)}; },
                                  [](uint8_t *p, const AffP<Fe> &r) { fe_store(p, r.x); fe_store(p + 32, r.y); });
    stats_flush();
    return rc;
}
void hc_opn_shape(size_t nbase, size_t n, size_t *out2) { opn_shape(nbase, n, out2, out2 + 1); }
// The data-dependent routines of fe29.hip.hpp on RAW limbs (tests/limb_cases.py, tests/test_field_primitives.py): n rows of nine int32,
// given the interval class the caller names — limbs 0..7 within +-(2^29 + slack) (fe_cyclo_out, op 6: within [-slack, 2^29 + slack], the
// class its comment states for t and x), the top limb as it stands, |value| <= vb p with vb[2 i] for row i of a and vb[2 i + 1] for
// row i of b (only op 6 reads b).  op: 0 fe_norm, 1 fe_mul8_norm, 2 fe_halve, 3 fe_reduce, 4 fe_reduce_arith, 5 fe_reduce_arith_norm,
// 6 fe_cyclo_out(a, b), 7 fe_canonical, 8 fe_is_zero (flags_out[i]; its out row is zero).  Every routine checks its own input class and
// that its tracked intervals hold the actual output (check_limbs).  -1: no such op.
static Fe fe_raw_class(const int32_t *w, double lo, double hi, double vb) {
    Fe r;
    for (int i = 0; i < NL; i++) { r.v[i] = w[i]; r.lo[i] = lo; r.hi[i] = hi; }
    r.lo[NL - 1] = r.hi[NL - 1] = (double)w[NL - 1];
    r.vb = vb;
    check_limbs(r, "raw limb outside the class the caller named");
    return r;
}
int hc_fe_primitive(int op, const int32_t *a_limbs, const int32_t *b_limbs, size_t n, int slack, const double *vb, int32_t *out_limbs, int32_t *flags_out) {
    if (op < 0 || op > 8) return -1;
    const double hi = 536870912.0 + (double)slack, lo = op == 6 ? -(double)slack : -hi;
    for (size_t i = 0; i < n; i++) {
        const Fe a = fe_raw_class(a_limbs + NL * i, lo, hi, vb[2 * i]);
        Fe r = fe_zero();
        int flag = 0;
        switch (op) {
        case 0: r = fe_norm(a); break;
        case 1: r = fe_mul8_norm(a); break;
        case 2: r = fe_halve(a); break;
        case 3: r = fe_reduce(a); break;
        case 4: r = fe_reduce_arith(a); break;
        case 5: r = fe_reduce_arith_norm(a); break;
        case 6: r = fe_cyclo_out(a, fe_raw_class(b_limbs + NL * i, lo, hi, vb[2 * i + 1])); break;
        case 7: r = fe_canonical(a); break;
        default: flag = fe_is_zero(a) ? 1 : 0; break;
        }
        check_limbs(r, "fe primitive output");
        for (int j = 0; j < NL; j++) out_limbs[NL * i + j] = r.v[j];
        flags_out[i] = flag;
    }
    stats_flush();
    return 0;
}
}
