// Stand-alone driver of yasph2d_amd/csrc/sphx_contour_merge.hpp (no GPU, no HIP): the stable K-way merge of the tiles' segment lists by
// cell word, and the apron assembly — which border word of which tile fills each apron node of a tile's padded window.  Built by
// tests/test_contour_multi_host.py with -ffp-contract=off and -fsanitize=address,undefined and run directly.
//   contour_merge_driver merge   -> "ok <cases>": seeded parts with disjoint cell sets (saddle cells, empty parts, no part at all) against a
//                                   stable sort of their concatenation; truncation at a capacity with sentinels behind it
//   contour_merge_driver apron   -> "ok <cases>": windows of 2 strips in x, 3 strips in y and a 2 x 2 grid with its own y cuts per column,
//                                   over fine, coarse and one-node-wide lattices: every apron node is found in exactly one border and
//                                   carries that node's word; a window taken away or doubled is reported
//   contour_merge_driver apron <gmin.x> <gmin.y> <h>   the same on another cell grid (fp32 bit patterns, hex): the lattices keep their place
//                                   and spacing in cells (cell 5000 is where x = 0 lay), the cuts stay the cell indices they are
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sphx_contour_merge.hpp"

namespace ch = sphx_contour_host;
namespace sh = sphx_sample_host;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t below(uint32_t n) { return n ? (uint32_t)(rnd() % n) : 0u; }

#define REQUIRE(cond, ...)                 \
    do {                                   \
        if (!(cond)) {                     \
            std::printf("FAIL " __VA_ARGS__); \
            std::printf("\n");             \
            return 1;                      \
        }                                  \
    } while (0)

// ---- merge ------------------------------------------------------------------------------------------------------------------------------
struct Part {
    std::vector<float> seg;
    std::vector<uint32_t> cell;
    std::vector<int32_t> tile;
};

static int run_merge() {
    uint32_t cases = 0;
    for (uint32_t round = 0; round < 120; ++round) {
        const uint32_t n_parts = round < 4 ? 0u : 1u + below(6);
        const uint32_t n_cells = round % 7 == 0 ? below(4) : 20u + below(400);
        std::vector<Part> parts(n_parts);
        const uint32_t empty_part = n_parts > 1 && round % 3 == 0 ? below(n_parts) : n_parts;  // this one gets nothing
        uint32_t saddles = 0;
        // ascending cell words, each given to one part; every fifth or so is a saddle cell: two entries with one word
        uint32_t word = below(50);
        for (uint32_t c = 0; c < n_cells && n_parts; ++c, word += 1u + below(9)) {
            uint32_t p = below(n_parts);
            if (p == empty_part) p = (p + 1u) % n_parts;
            const uint32_t n = below(5) == 0 ? 2u : 1u;
            saddles += n == 2u;
            for (uint32_t k = 0; k < n; ++k) {
                for (int j = 0; j < 4; ++j) parts[p].seg.push_back((float)(rnd() >> 40));
                parts[p].cell.push_back(word);
                parts[p].tile.push_back((int32_t)p);
            }
        }
        // the expected order: a stable sort of the concatenation by cell word
        struct Ref {
            uint32_t cell, part, at;
        };
        std::vector<Ref> ref;
        for (uint32_t p = 0; p < n_parts; ++p)
            for (uint32_t j = 0; j < parts[p].cell.size(); ++j) ref.push_back(Ref{parts[p].cell[j], p, j});
        std::stable_sort(ref.begin(), ref.end(), [](const Ref& a, const Ref& b) { return a.cell < b.cell; });
        std::vector<ch::MergePart> mp(n_parts);
        for (uint32_t p = 0; p < n_parts; ++p)
            mp[p] = ch::MergePart{parts[p].seg.data(), parts[p].cell.data(), round % 2 ? parts[p].tile.data() : nullptr, (int32_t)p, (uint32_t)parts[p].cell.size()};
        const uint32_t total = (uint32_t)ref.size();
        const uint32_t caps[4] = {total, total + 5u, total ? total - 1u : 0u, total / 2u};
        for (uint32_t cap : caps) {
            // outputs of exactly `cap` entries and a sentinel tail the merge must not touch (the sanitizer guards what lies behind)
            const uint32_t tail = 3u;
            std::vector<float> seg(4 * (size_t)(cap + tail), -7.0f);
            std::vector<uint32_t> cell(cap + tail, 0xDEADBEEFu);
            std::vector<int32_t> tile(cap + tail, -77);
            const uint32_t wrote = ch::merge(mp.data(), n_parts, cap, ch::MergeOut{seg.data(), cell.data(), tile.data()});
            REQUIRE(wrote == std::min(cap, total), "round %u cap %u: wrote %u of %u", round, cap, wrote, total);
            for (uint32_t k = 0; k < wrote; ++k) {
                const Ref& r = ref[k];
                REQUIRE(cell[k] == r.cell && tile[k] == (int32_t)r.part, "round %u cap %u entry %u: cell %u tile %d, want %u %u", round, cap, k, cell[k], tile[k],
                        r.cell, r.part);
                REQUIRE(std::memcmp(seg.data() + 4 * (size_t)k, parts[r.part].seg.data() + 4 * (size_t)r.at, 16) == 0, "round %u cap %u entry %u: segment", round,
                        cap, k);
            }
            for (uint32_t k = wrote; k < cap + tail; ++k)
                REQUIRE(cell[k] == 0xDEADBEEFu && tile[k] == -77 && seg[4 * (size_t)k] == -7.0f && seg[4 * (size_t)k + 3] == -7.0f,
                        "round %u cap %u: entry %u behind the written ones was touched", round, cap, k);
            // NULL outputs are skipped
            REQUIRE(ch::merge(mp.data(), n_parts, cap, ch::MergeOut{nullptr, cell.data(), nullptr}) == wrote, "round %u: NULL outputs", round);
            ++cases;
        }
        if (round == 119) REQUIRE(saddles > 0, "no saddle cell in the last round");
    }
    std::printf("ok %u\n", cases);
    return 0;
}

// ---- apron assembly -----------------------------------------------------------------------------------------------------------------------
struct CellRect {
    uint32_t x0, x1, y0, y1;
};
struct LatticeCase {
    const char* name;
    float x0, y0, dx, dy;
    uint32_t nx, ny;
};

static float GMIN[2] = {-100.0f, -100.0f}, H = 0.02f;
static float CELL_INV = 1.0f / H;
static bool g_other_grid = false;

static float from_bits(const char* hex) {
    const uint32_t u = (uint32_t)std::strtoul(hex, nullptr, 16);
    float f;
    std::memcpy(&f, &u, sizeof(f));
    return f;
}

// a lattice written down for grid_min (-100, -100), h = 0.02, moved to the grid in use: the same cells, the same spacing in cells
static float moved(float v, int axis) { return g_other_grid ? GMIN[axis] + (5000.0f + v / 0.02f) * H : v; }
static float scaled(float d) { return g_other_grid ? d / 0.02f * H : d; }

static uint32_t g_reported = 0;  // apron look-ups that named a node of a window taken away
static uint32_t node_word(uint32_t ix, uint32_t iy) { return 0x40000000u + iy * 4099u + ix; }

static int check_layout(const char* lname, const std::vector<CellRect>& rects, const LatticeCase& written, uint32_t& cases, uint32_t& empty_tiles, uint32_t& apron_nodes) {
    const LatticeCase L = {written.name, moved(written.x0, 0), moved(written.y0, 1), scaled(written.dx), scaled(written.dy), written.nx, written.ny};
    const uint32_t n = (uint32_t)rects.size();
    std::vector<ch::Window> wins(n);
    for (uint32_t k = 0; k < n; ++k)
        wins[k] = sh::lattice_window(L.x0, L.y0, L.dx, L.dy, L.nx, L.ny, GMIN[0], GMIN[1], CELL_INV, rects[k].x0, rects[k].x1, rects[k].y0, rects[k].y1);
    REQUIRE(ch::windows_cover(wins.data(), n, L.nx, L.ny), "%s / %s: the windows do not cover the lattice", lname, L.name);
    const std::vector<size_t> off = ch::border_offsets(wins.data(), n);
    // the borders as the tiles would pack them, every node carrying its own word
    std::vector<uint32_t> borders(off[n], 0u);
    for (uint32_t k = 0; k < n; ++k) {
        const ch::Window& w = wins[k];
        if (!w.points()) {
            ++empty_tiles;
            REQUIRE(off[k + 1] == off[k], "%s / %s: an empty window has a border", lname, L.name);
            continue;
        }
        for (uint32_t i = 0; i < w.w(); ++i) borders[off[k] + i] = node_word(w.ix0 + i, w.iy0);
        for (uint32_t j = 0; j < w.h(); ++j) borders[off[k] + w.w() + j] = node_word(w.ix0, w.iy0 + j);
    }
    uint64_t cut = 0;
    std::vector<size_t> idx;
    for (uint32_t k = 0; k < n; ++k) {
        const ch::Window& w = wins[k];
        uint32_t bx = 0, by = 0;
        const int rc = ch::apron_indices(wins.data(), off.data(), n, L.nx, L.ny, k, idx, &bx, &by);
        REQUIRE(rc == ch::NODE_OK, "%s / %s: apron node (%u, %u) of tile %u: error %d", lname, L.name, bx, by, k, rc);
        REQUIRE(idx.size() == ch::apron_words(w, L.nx, L.ny), "%s / %s: tile %u has %zu apron words", lname, L.name, k, idx.size());
        // the expected nodes in the unpack order, and each found in exactly one tile's border
        std::vector<uint32_t> want;
        const uint32_t ax = ch::apron_ax(w, L.nx), ay = ch::apron_ay(w, L.ny);
        if (ax)
            for (uint32_t iy = w.iy0; iy < w.iy1; ++iy) want.push_back(node_word(w.ix1, iy));
        if (ay)
            for (uint32_t ix = w.ix0; ix < w.ix1; ++ix) want.push_back(node_word(ix, w.iy1));
        if (ax & ay) want.push_back(node_word(w.ix1, w.iy1));
        REQUIRE(want.size() == idx.size(), "%s / %s: tile %u apron size", lname, L.name, k);
        for (size_t i = 0; i < idx.size(); ++i) {
            REQUIRE(idx[i] < borders.size() && borders[idx[i]] == want[i], "%s / %s: tile %u apron word %zu is another node's", lname, L.name, k, i);
            uint32_t holders = 0;
            for (uint32_t t = 0; t < n; ++t) {
                bool has = false;
                for (size_t j = off[t]; j < off[t + 1]; ++j) has = has || borders[j] == want[i];
                holders += has;
            }
            REQUIRE(holders == 1u, "%s / %s: an apron node of tile %u is in %u borders", lname, L.name, k, holders);
            REQUIRE(!(idx[i] >= off[k] && idx[i] < off[k + 1]), "%s / %s: tile %u finds an apron node in its own border", lname, L.name, k);
        }
        apron_nodes += (uint32_t)idx.size();
        cut += ch::window_cells(w, L.nx, L.ny);
    }
    const uint64_t all_cells = L.nx >= 2u && L.ny >= 2u ? (uint64_t)(L.nx - 1u) * (L.ny - 1u) : 0u;
    REQUIRE(cut == all_cells, "%s / %s: the tiles cut %llu of %llu cells", lname, L.name, (unsigned long long)cut, (unsigned long long)all_cells);
    ++cases;
    // a window taken away: the lattice is no longer covered, and a neighbour's apron look-up names the missing node
    for (uint32_t gone = 0; gone < n; ++gone) {
        if (!wins[gone].points()) continue;
        std::vector<ch::Window> holed = wins;
        holed[gone] = ch::Window{0, 0, 0, 0};
        REQUIRE(!ch::windows_cover(holed.data(), n, L.nx, L.ny), "%s / %s: a missing window went unnoticed", lname, L.name);
        const std::vector<size_t> hoff = ch::border_offsets(holed.data(), n);
        for (uint32_t k = 0; k < n; ++k) {
            if (k == gone) continue;
            uint32_t bx = 0, by = 0;
            const int rc = ch::apron_indices(holed.data(), hoff.data(), n, L.nx, L.ny, k, idx, &bx, &by);
            const ch::Window& g = wins[gone];
            if (rc == ch::NODE_IN_NO_WINDOW) {
                ++g_reported;
                REQUIRE(bx >= g.ix0 && bx < g.ix1 && by >= g.iy0 && by < g.iy1, "%s / %s: the reported node is not the missing window's", lname, L.name);
            } else {
                REQUIRE(rc == ch::NODE_OK, "%s / %s: error %d with a window missing", lname, L.name, rc);
            }
        }
        ++cases;
    }
    // a window doubled: a node in two windows is reported
    if (n >= 2 && wins[0].points() && wins[1].points()) {
        std::vector<ch::Window> dbl = wins;
        dbl[0] = wins[1];
        const std::vector<size_t> doff = ch::border_offsets(dbl.data(), n);
        size_t at = 0;
        REQUIRE(ch::border_index(dbl.data(), doff.data(), n, wins[1].ix0, wins[1].iy0, &at) == ch::NODE_IN_SEVERAL, "%s / %s: a doubled window went unnoticed", lname,
                L.name);
        ++cases;
    }
    return 0;
}

static int run_apron() {
    // the cells of x = 0 .. 2 and y = 0 .. 1 start at (0 - GMIN) / H = 5000
    const std::vector<CellRect> strips_x = {{0u, 5030u, 0u, 65536u}, {5030u, 65536u, 0u, 65536u}};
    const std::vector<CellRect> strips_y = {{0u, 65536u, 0u, 5011u}, {0u, 65536u, 5011u, 5013u}, {0u, 65536u, 5013u, 65536u}};  // a thin one in the middle
    const std::vector<CellRect> grid = {{0u, 5027u, 0u, 5009u}, {0u, 5027u, 5009u, 65536u}, {5027u, 65536u, 0u, 5021u}, {5027u, 65536u, 5021u, 65536u}};
    const std::vector<CellRect> thin_x = {{0u, 5020u, 0u, 65536u}, {5020u, 5022u, 0u, 65536u}, {5022u, 65536u, 0u, 65536u}};
    const LatticeCase lattices[] = {
        {"fine", -0.05f, -0.03f, 0.012f, 0.012f, 130u, 70u},      // spacing < h
        {"fine, unequal", 0.1f, 0.05f, 0.007f, 0.015f, 97u, 33u},
        {"coarse", -0.1f, -0.1f, 0.07f, 0.065f, 30u, 12u},        // spacing > 3 h: a thin tile owns no node
        {"one node wide", 0.61f, -0.02f, 0.012f, 0.012f, 1u, 80u},
        {"one node high", -0.02f, 0.23f, 0.012f, 0.012f, 120u, 1u},
        {"one node", 0.3f, 0.3f, 0.012f, 0.012f, 1u, 1u},
        {"two by two", 0.59f, 0.17f, 0.012f, 0.012f, 2u, 2u},
        {"inside one tile", 0.05f, 0.02f, 0.01f, 0.01f, 20u, 10u},
    };
    uint32_t cases = 0, empty_tiles = 0, apron_nodes = 0;
    const std::pair<const char*, const std::vector<CellRect>*> layouts[] = {
        {"2 strips in x", &strips_x}, {"3 strips in y", &strips_y}, {"2 x 2 grid", &grid}, {"3 strips in x, thin middle", &thin_x}};
    for (const auto& lay : layouts)
        for (const LatticeCase& L : lattices)
            if (check_layout(lay.first, *lay.second, L, cases, empty_tiles, apron_nodes)) return 1;
    REQUIRE(empty_tiles > 0, "no case had a tile without a node");
    REQUIRE(g_reported > 10, "only %u look-ups reported a missing window", g_reported);
    REQUIRE(apron_nodes > 1000, "only %u apron nodes were looked up", apron_nodes);
    std::printf("ok %u\n", cases);
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "merge") return run_merge();
    if (mode == "apron" && argc >= 5) {
        GMIN[0] = from_bits(argv[2]), GMIN[1] = from_bits(argv[3]), H = from_bits(argv[4]);
        CELL_INV = 1.0f / H;
        g_other_grid = true;
    }
    if (mode == "apron") return run_apron();
    std::fprintf(stderr, "usage: contour_merge_driver merge | apron [gmin.x gmin.y h as fp32 bit patterns]\n");
    return 2;
}
