// Host sanitizer run of csrc/formula29.hip.hpp: the per-lane bodies of k_fr_lsss_from_formula and k_formula_select as the kernels run them,
// on malformed rows, on 127-node formulas and on rows of arbitrary codes, with every buffer (the LDS stand-in among them) an exact-size heap
// block, so that AddressSanitizer sees any access outside it and UBSan any shift or conversion out of range.
//
// build and run (host only):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o tools/formula_san tools/formula_san.cpp && tools/formula_san
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../gopairingbasedcryptography_amd/csrc/formula29.hip.hpp"

using namespace gpbc;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

struct Built { std::vector<uint8_t> matrix, ok; std::vector<int64_t> rho; std::vector<uint32_t> dims; };

// the kernel's three phases, workgroup by workgroup; a barrier = the end of a loop over the lanes
static Built build(const std::vector<int64_t> &nodes, size_t n_nodes, size_t rows, size_t cols, bool wide) {
    const size_t k = nodes.size() / n_nodes;
    Built b;
    b.matrix.assign(k * rows * cols * 32 + 16, 0xA5); b.ok.assign(k, 0xA5); b.rho.assign(k * rows, 0x5A5A); b.dims.assign(k * 2, 0xA5A5);
    uint8_t *m = b.matrix.data() + (wide ? (16 - (uintptr_t)b.matrix.data() % 16) % 16 : 1);      // 16-byte aligned, or odd
    const FormulaGeom g = formula_build_geometry(n_nodes, rows, cols, wide);
    const FormulaOut o{m, (uint8_t *)b.rho.data(), (uint8_t *)b.dims.data(), b.ok.data(), rows * cols * 32, rows * sizeof(int64_t), 2 * sizeof(uint32_t)};
    for (size_t block = 0; block < formula_grid(g, k); block++) {
        std::vector<uint32_t> lds(FORMULA_BUILD_WORDS);
        const auto getw = [&](uint32_t off) { return lds.at(off); };
        const auto putw = [&](uint32_t off, uint32_t v) { lds.at(off) = v; };
        for (uint32_t lane = 0; lane < FORMULA_WAVE; lane++) formula_stage(g, (uint32_t)block, lane, k, nodes.data(), putw);
        for (uint32_t lane = 0; lane < FORMULA_WAVE; lane++) formula_build_walk(g, (uint32_t)block, lane, k, getw, putw);
        for (uint32_t lane = 0; lane < FORMULA_WAVE; lane++)
            formula_build_write(g, (uint32_t)block, lane, k, getw,
                                [&](size_t item, uint32_t p, const uint32_t (&w)[4]) { formula_store_piece(g, o, item, p, w); },
                                [&](size_t item, uint32_t x, int64_t a) { formula_store_rho(o, item, x, a); },
                                [&](size_t item, bool ok, uint32_t nr, uint32_t nc) { formula_store_done(o, item, ok, nr, nc); });
    }
    std::memmove(b.matrix.data(), m, k * rows * cols * 32);
    return b;
}
struct Selected { std::vector<uint8_t> chosen, ok; };
static Selected select(const std::vector<int64_t> &nodes, size_t n_nodes, const std::vector<uint8_t> &held, size_t rows) {
    const size_t k = held.size() / rows, n_formulas = nodes.size() / n_nodes;
    Selected s;
    s.chosen.assign(k * rows, 0xA5); s.ok.assign(k, 0xA5);
    const FormulaGeom g = formula_select_geometry(n_nodes, rows, n_formulas == 1 && k > 1);
    for (size_t block = 0; block < formula_grid(g, k); block++) {
        std::vector<uint32_t> lds(FORMULA_SELECT_WORDS);
        for (uint32_t lane = 0; lane < FORMULA_WAVE; lane++) formula_stage(g, (uint32_t)block, lane, k, nodes.data(), [&](uint32_t off, uint32_t v) { lds.at(off) = v; });
        for (uint32_t lane = 0; lane < FORMULA_WAVE; lane++)
            formula_select_lane(g, (uint32_t)block, lane, k, [&](uint32_t off) { return lds.at(off); }, held.data(),
                                [&](size_t item, bool ok, uint64_t chosen) { formula_store_chosen(g, s.chosen.data(), s.ok.data(), item, ok, chosen); });
    }
    return s;
}
static std::vector<int64_t> deep(int64_t gate, int leaves, bool left, size_t n_nodes) {
    std::vector<int64_t> r;
    if (left) { for (int i = 1; i < leaves; i++) r.push_back(gate); for (int i = 0; i < leaves; i++) r.push_back(100 + i); }
    else { for (int i = 1; i < leaves; i++) { r.push_back(gate); r.push_back(100 + i); } r.push_back(100); }
    r.resize(n_nodes, FORMULA_END);
    return r;
}
static uint64_t rng_state = 29;
static uint64_t rng() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return rng_state >> 17; }

int main() {
    const int64_t A = FORMULA_AND, O = FORMULA_OR, E = FORMULA_END, MIN = INT64_MIN;
    // malformed rows of seven codes; the first row is (1 and (2 or 3))
    const std::vector<std::vector<int64_t>> bad = {{A, 1, O, 2, 3, E, E}, {A, 1, O, 2, 3, 4, A}, {O, E, E, E, E, E, E}, {A, 1, E, 2, E, E, E}, {O, 1, 2, E, 3, E, E},
                                                   {5, A, E, E, E, E, E}, {A, -4, 2, E, E, E, E}, {MIN, E, E, E, E, E, E}, {O, 1, 2, MIN, E, E, E}, {E, E, E, E, E, E, E},
                                                   {A, A, 1, 2, E, E, E}, {A, A, A, A, A, A, A}, {O, O, O, O, O, O, O}};
    std::vector<int64_t> rows7;
    for (const auto &r : bad) rows7.insert(rows7.end(), r.begin(), r.end());
    for (int wide = 0; wide < 2; wide++) {
        const Built b = build(rows7, 7, 4, 3, wide != 0);
        EXPECT(b.ok[0] == 1 && b.dims[0] == 3 && b.dims[1] == 2 && b.rho[0] == 1 && b.rho[2] == 3 && b.rho[3] == -1);
        for (size_t j = 1; j < bad.size(); j++) {
            EXPECT(b.ok[j] == 0 && b.dims[2 * j] == 0 && b.dims[2 * j + 1] == 0);
            for (size_t x = 0; x < 4; x++) EXPECT(b.rho[4 * j + x] == -1);
            for (size_t i = 0; i < 4 * 3 * 32; i++) EXPECT(b.matrix[j * 4 * 3 * 32 + i] == 0);
        }
    }
    const Selected s7 = select(rows7, 7, std::vector<uint8_t>(bad.size() * 4, 1), 4);
    EXPECT(s7.ok[0] == 1 && s7.chosen[0] == 1 && s7.chosen[1] == 1 && s7.chosen[2] == 0 && s7.chosen[3] == 0);
    for (size_t j = 1; j < bad.size(); j++) EXPECT(s7.ok[j] == 0 && !s7.chosen[4 * j] && !s7.chosen[4 * j + 1] && !s7.chosen[4 * j + 2] && !s7.chosen[4 * j + 3]);
    // 127 nodes: the deepest stacks, the last column, 127 gates in a row, 127 leaves in a row
    std::vector<int64_t> big;
    for (const auto &r : {deep(A, 64, true, 127), deep(A, 64, false, 127), deep(O, 64, true, 127), deep(O, 64, false, 127), std::vector<int64_t>(127, A), std::vector<int64_t>(127, O),
                          std::vector<int64_t>(127, 7), deep(A, 63, true, 127)})
        big.insert(big.end(), r.begin(), r.end());
    big[7 * 127 + 125] = 9;                                                       // the last: one node too many behind a whole tree
    for (int wide = 0; wide < 2; wide++) {
        const Built b = build(big, 127, 64, 64, wide != 0);
        EXPECT(b.ok[0] == 1 && b.dims[0] == 64 && b.dims[1] == 64 && b.ok[1] == 1 && b.dims[3] == 64 && b.ok[2] == 1 && b.dims[5] == 1 && b.ok[3] == 1);
        EXPECT(b.ok[4] == 0 && b.ok[5] == 0 && b.ok[6] == 0 && b.ok[7] == 0);
        const Built small = build(big, 127, 63, 64, wide != 0), narrow = build(big, 127, 64, 63, wide != 0);
        EXPECT(small.ok[0] == 0 && small.ok[2] == 0 && narrow.ok[0] == 0 && narrow.ok[1] == 0 && narrow.ok[2] == 1);
    }
    std::vector<uint8_t> all(8 * 64, 1);
    all[63] = 0;                                                                  // the left-deep AND without its last leaf
    const Selected sb = select(big, 127, all, 64);
    EXPECT(sb.ok[0] == 0 && sb.ok[1] == 1 && sb.ok[2] == 1 && sb.ok[3] == 1 && sb.ok[4] == 0 && sb.ok[5] == 0 && sb.ok[6] == 0 && sb.ok[7] == 0);
    EXPECT(sb.chosen[64 + 0] == 1 && sb.chosen[64 + 63] == 1 && sb.chosen[2 * 64] == 1 && sb.chosen[2 * 64 + 1] == 0);
    const Selected shared = select(deep(O, 64, false, 127), 127, all, 64);
    EXPECT(shared.ok[0] == 1 && shared.ok[7] == 1);
    // rows of arbitrary codes: nothing may be touched outside the buffers, whatever the verdicts
    for (int round = 0; round < 200; round++) {
        const size_t n_nodes = 1 + rng() % 127, rows = 1 + rng() % 64, cols = 1 + rng() % 64, k = 1 + rng() % 9;
        std::vector<int64_t> nodes(k * n_nodes);
        for (auto &c : nodes) { const uint64_t r = rng() % 16; c = r < 6 ? (int64_t)(rng() % 50) : r < 10 ? A : r < 14 ? O : r == 14 ? E : (int64_t)rng() * (int64_t)(rng() % 3 - 1); }
        std::vector<uint8_t> held(k * rows);
        for (auto &h : held) h = (uint8_t)(rng() % 3);
        const Built b = build(nodes, n_nodes, rows, cols, round % 2 != 0);
        const Selected s = select(nodes, n_nodes, held, rows);
        for (size_t j = 0; j < k; j++) EXPECT(b.ok[j] <= 1 && s.ok[j] <= 1 && (b.ok[j] || !s.ok[j] || b.dims[2 * j] == 0));
    }
    if (failures) { std::printf("formula_san: %d failures\n", failures); return 1; }
    std::printf("formula_san: clean\n");
    return 0;
}
