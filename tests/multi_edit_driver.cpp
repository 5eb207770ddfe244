// multi_edit_driver.cpp — the host rules of an edit of a tiled run (yasph2d_amd/csrc/sphx_multi_edit.hpp) as a stand-alone program: routing
// of new records to the tiles that own their cells, the id counter, the check of the positions.  Built by tests/test_multi_edit_host.py
// with the address and undefined-behaviour sanitizers; prints "ok <checks>" or the first failed check.
//   multi_edit_driver <routing|ids|positions|empty> [<gmin.x> <gmin.y> <h>]    the grid of the hand cases as fp32 bit patterns (hex);
//                                                                              default: grid_min (-100, -100), h = 0.02
//   multi_edit_driver route <gmin> <h> <n_rects> {x0 x1 y0 y1}... {x y}...     -> the owners, one per record (for the numpy restatement)
//   multi_edit_driver routebits <gmin.x> <gmin.y> <h> <n_rects> {x0 x1 y0 y1}... {x y}...   the same, every float as its fp32 bit pattern
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "sphx_multi_edit.hpp"

namespace me = sphx_multi_edit;

static int checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++checks;                                                          \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static float GMIN[2] = {-100.0f, -100.0f};
static float H = 0.02f;
static float INV = 1.0f / H;

static float from_bits(const char* hex) {
    const uint32_t u = (uint32_t)std::strtoul(hex, nullptr, 16);
    float f;
    std::memcpy(&f, &u, sizeof(f));
    return f;
}

// the world coordinate of the low edge of cell c along `axis`, nudged into the cell (fp32 of -100 + c * 0.02 may round to either side)
static float in_cell(uint32_t c, float frac = 0.5f, int axis = 0) { return GMIN[axis] + ((float)c + frac) * H; }
static float in_cell_y(uint32_t c, float frac = 0.5f) { return in_cell(c, frac, 1); }

static std::vector<int> owners(const std::vector<float>& xy, const std::vector<me::CellRect>& rects) {
    std::vector<int> o;
    me::route(xy.data(), (uint32_t)(xy.size() / 2), GMIN, INV, rects.data(), (int)rects.size(), o);
    return o;
}

static int routing() {
    // three strips along x cut at cells 5000 and 5040
    const std::vector<me::CellRect> strips = {{0u, 5000u, 0u, 65536u}, {5000u, 5040u, 0u, 65536u}, {5040u, 65536u, 0u, 65536u}};
    {
        const std::vector<float> xy = {in_cell(4999), in_cell_y(10), in_cell(5000, 0.01f), in_cell_y(77), in_cell(5039, 0.99f), in_cell_y(5040), in_cell(5040, 0.01f), in_cell_y(0),
                                       in_cell(65535), in_cell_y(65535), -1.0e9f, 5.0f, 1.0e9f, -1.0e9f};
        const std::vector<int> o = owners(xy, strips);
        CHECK(o.size() == 7);
        CHECK(o[0] == 0);  // the last cell of the first strip
        CHECK(o[1] == 1);  // just above the cut: the cut's own cell, the high side
        CHECK(o[2] == 1);
        CHECK(o[3] == 2);
        CHECK(o[4] == 2);  // the far corner cell
        CHECK(o[5] == 0);  // left of the grid: cell 0
        CHECK(o[6] == 2);  // right of it: cell 65535 (x), cell 0 (y)
    }
    // the cell of a position is what the device computes: (v - gmin) * (1 / h) in fp32, truncated
    for (int axis = 0; axis < 2; ++axis)
        for (uint32_t c : {0u, 1u, 4999u, 5000u, 5017u, 65534u, 65535u}) {
            CHECK(me::cell_coord(in_cell(c, 0.5f, axis), GMIN[axis], INV) == c);
            const float v = in_cell(c, 0.5f, axis);
            const float f = (v - GMIN[axis]) * INV;
            CHECK(me::cell_coord(v, GMIN[axis], INV) == (f >= 65535.0f ? 65535u : (uint32_t)f));
        }
    CHECK(me::cell_coord(std::numeric_limits<float>::quiet_NaN(), GMIN[0], INV) == 0u);
    CHECK(me::cell_coord(-std::numeric_limits<float>::infinity(), GMIN[0], INV) == 0u);
    CHECK(me::cell_coord(std::numeric_limits<float>::infinity(), GMIN[0], INV) == 65535u);
    // a 2 x 2 grid: columns cut at x cell 5017, the left column cut at y cell 5059, the right one at 5061; rank = ix * 2 + iy
    const std::vector<me::CellRect> grid = {{0u, 5017u, 0u, 5059u}, {0u, 5017u, 5059u, 65536u}, {5017u, 65536u, 0u, 5061u}, {5017u, 65536u, 5061u, 65536u}};
    {
        struct Case {
            uint32_t cx, cy;
            int want;
        };
        const Case cases[] = {{5016, 5058, 0}, {5016, 5059, 1}, {5017, 5059, 2}, {5017, 5060, 2}, {5017, 5061, 3}, {5016, 5060, 1},  // around the crossing
                              {0, 0, 0},       {0, 65535, 1},   {65535, 0, 2},   {65535, 65535, 3},                                    // the corner cells
                              {5017, 0, 2},    {5016, 65535, 1}};
        std::vector<float> xy;
        for (const Case& c : cases) {
            xy.push_back(in_cell(c.cx));
            xy.push_back(in_cell_y(c.cy));
        }
        const std::vector<int> o = owners(xy, grid);
        for (size_t k = 0; k < sizeof(cases) / sizeof(cases[0]); ++k) {
            CHECK(me::cell_coord(xy[2 * k], GMIN[0], INV) == cases[k].cx && me::cell_coord(xy[2 * k + 1], GMIN[1], INV) == cases[k].cy);
            CHECK(o[k] == cases[k].want);
            CHECK(me::owner_of(cases[k].cx, cases[k].cy, grid.data(), 4) == cases[k].want);
        }
    }
    // every cell has exactly one owner in a layout; rectangles that leave a cell out say so
    for (uint32_t cx = 5010; cx < 5025; ++cx)
        for (uint32_t cy = 5050; cy < 5070; ++cy) {
            int n = 0;
            for (const me::CellRect& r : grid) n += me::in_rect(cx, cy, r) ? 1 : 0;
            CHECK(n == 1);
        }
    const std::vector<me::CellRect> gap = {{0u, 10u, 0u, 65536u}, {20u, 65536u, 0u, 65536u}};
    CHECK(me::owner_of(15, 3, gap.data(), 2) == -1 && me::owner_of(9, 3, gap.data(), 2) == 0 && me::owner_of(20, 3, gap.data(), 2) == 1);
    {
        const std::vector<float> xy = {in_cell(15), in_cell_y(3), in_cell(25), in_cell_y(3), in_cell(15), in_cell_y(3)};
        const std::vector<int> o = owners(xy, gap);
        CHECK(o[0] == -1 && o[1] == 1 && o[2] == -1);  // (the "try the last owner first" shortcut does not adopt a record nobody owns)
    }
    // the owner does not depend on the order of the records (the shortcut is only a shortcut)
    {
        std::vector<float> xy;
        uint32_t s = 12345u;
        for (int k = 0; k < 500; ++k) {
            s = s * 1664525u + 1013904223u;
            xy.push_back(in_cell(5000u + (s >> 8) % 40u));
            s = s * 1664525u + 1013904223u;
            xy.push_back(in_cell_y(5040u + (s >> 8) % 40u));
        }
        const std::vector<int> o = owners(xy, grid);
        for (int k = 0; k < 500; ++k) CHECK(o[k] == me::owner_of(me::cell_coord(xy[2 * k], GMIN[0], INV), me::cell_coord(xy[2 * k + 1], GMIN[1], INV), grid.data(), 4));
    }
    return 0;
}

static int ids() {
    // after an upload without ids: n
    CHECK(me::counter_after(nullptr, 0) == 0 && me::counter_after(nullptr, 4050) == 4050);
    // with ids (gaps, any order): 1 + the greatest; an empty set: 0
    const uint32_t some[] = {7u, 3u, 1000u, 12u};
    CHECK(me::counter_after(some, 4) == 1001 && me::counter_after(some, 2) == 8 && me::counter_after(some, 0) == 0);
    const uint32_t top[] = {0x7FFFFFFEu};
    CHECK(me::counter_after(top, 1) == 0x7FFFFFFFull);
    const uint32_t beyond[] = {0xFFFFFFFFu};
    CHECK(me::counter_after(beyond, 1) == 0x100000000ull);
    // taking ids
    uint64_t c = 4050;
    uint32_t first = 99;
    CHECK(me::take_ids(c, 81, &first) && first == 4050 && c == 4131);
    CHECK(me::take_ids(c, 0, &first) && first == 4131 && c == 4131);
    CHECK(me::take_ids(c, 5, nullptr) && c == 4136);
    // the last id is 2^31 - 1
    c = me::ID_LIMIT - 2;
    CHECK(!me::take_ids(c, 3, &first) && c == me::ID_LIMIT - 2 && first == 0x7FFFFFFEu);  // nothing taken
    CHECK(me::take_ids(c, 2, &first) && first == 0x7FFFFFFEu && c == me::ID_LIMIT);
    CHECK(!me::take_ids(c, 1, &first) && c == me::ID_LIMIT && first == 0x80000000u);
    CHECK(me::take_ids(c, 0, &first) && first == 0x80000000u);  // n_new == 0 still reports
    c = 0x100000000ull;  // (an upload with ids beyond the limit)
    CHECK(!me::take_ids(c, 1, &first) && me::take_ids(c, 0, &first) && first == 0x80000000u);
    c = 0;
    CHECK(!me::take_ids(c, 0x80000001u, &first) && c == 0 && me::take_ids(c, 0x80000000u, &first) && first == 0 && c == me::ID_LIMIT);
    return 0;
}

static int positions() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float good[] = {0.0f, 1.0f, -3.5f, 1.0e30f, -0.0f, 1.0e-40f};
    CHECK(me::first_nonfinite(good, 3) == 3);
    for (float bad : {nan, inf, -inf})
        for (int at = 0; at < 6; ++at) {
            float xy[6];
            std::memcpy(xy, good, sizeof(xy));
            xy[at] = bad;
            CHECK(me::first_nonfinite(xy, 3) == (uint32_t)(at / 2));
            CHECK(me::first_nonfinite(xy, (uint32_t)(at / 2)) == (uint32_t)(at / 2));  // (not looked at: behind the end)
        }
    float two[] = {nan, 0.0f, 1.0f, inf};
    CHECK(me::first_nonfinite(two, 2) == 0);
    return 0;
}

static int empty() {
    // n_new == 0: nothing is read, nothing is routed, the counter stays
    std::vector<int> o = {1, 2, 3};
    const me::CellRect whole = {0u, 65536u, 0u, 65536u};
    me::route(nullptr, 0, GMIN, INV, &whole, 1, o);
    CHECK(o.empty());
    me::route(nullptr, 0, GMIN, INV, nullptr, 0, o);
    CHECK(o.empty());
    CHECK(me::first_nonfinite(nullptr, 0) == 0);
    uint64_t c = 17;
    uint32_t first = 0;
    CHECK(me::take_ids(c, 0, &first) && first == 17 && c == 17);
    // one record, no rectangle at all
    const float xy[] = {0.5f, 0.5f};
    me::route(xy, 1, GMIN, INV, nullptr, 0, o);
    CHECK(o.size() == 1 && o[0] == -1);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string what = argv[1];
    if (what == "route") {
        if (argc < 5) return 2;
        const float gmin[2] = {(float)std::atof(argv[2]), (float)std::atof(argv[2])};
        const float inv = 1.0f / (float)std::atof(argv[3]);
        const int nr = std::atoi(argv[4]);
        std::vector<me::CellRect> rects;
        int at = 5;
        for (int r = 0; r < nr && at + 3 < argc; ++r, at += 4)
            rects.push_back(me::CellRect{(uint32_t)std::strtoul(argv[at], nullptr, 10), (uint32_t)std::strtoul(argv[at + 1], nullptr, 10),
                                         (uint32_t)std::strtoul(argv[at + 2], nullptr, 10), (uint32_t)std::strtoul(argv[at + 3], nullptr, 10)});
        std::vector<float> xy;
        for (; at < argc; ++at) xy.push_back(std::strtof(argv[at], nullptr));
        std::vector<int> o;
        me::route(xy.data(), (uint32_t)(xy.size() / 2), gmin, inv, rects.data(), (int)rects.size(), o);
        for (int v : o) std::printf("%d\n", v);
        return 0;
    }
    if (what == "routebits") {
        if (argc < 6) return 2;
        const float gmin[2] = {from_bits(argv[2]), from_bits(argv[3])};
        const float inv = 1.0f / from_bits(argv[4]);
        const int nr = std::atoi(argv[5]);
        std::vector<me::CellRect> rects;
        int at = 6;
        for (int r = 0; r < nr && at + 3 < argc; ++r, at += 4)
            rects.push_back(me::CellRect{(uint32_t)std::strtoul(argv[at], nullptr, 10), (uint32_t)std::strtoul(argv[at + 1], nullptr, 10),
                                         (uint32_t)std::strtoul(argv[at + 2], nullptr, 10), (uint32_t)std::strtoul(argv[at + 3], nullptr, 10)});
        std::vector<float> xy;
        for (; at < argc; ++at) xy.push_back(from_bits(argv[at]));
        std::vector<int> o;
        me::route(xy.data(), (uint32_t)(xy.size() / 2), gmin, inv, rects.data(), (int)rects.size(), o);
        for (int v : o) std::printf("%d\n", v);
        return 0;
    }
    if (argc >= 5) {  // the grid of the hand cases
        GMIN[0] = from_bits(argv[2]), GMIN[1] = from_bits(argv[3]), H = from_bits(argv[4]);
        INV = 1.0f / H;
    }
    int rc = 2;
    if (what == "routing") rc = routing();
    if (what == "ids") rc = ids();
    if (what == "positions") rc = positions();
    if (what == "empty") rc = empty();
    if (rc == 0) std::printf("ok %d\n", checks);
    return rc;
}
