// render_merge_driver.cpp — the host side of the tiled picture, driven without a GPU and under the address and undefined-behaviour
// sanitizers (tests/test_render_multi_host.py builds it): yasph2d_amd/csrc/sphx_render_merge.hpp (the composite rule) and
// yasph2d_amd/csrc/sphx_render_window.hpp (the float-to-index conversion of a tile's window).  Every array is allocated at exactly its
// size, so an index outside it is reported.
//   render_merge_driver merge    the fold against a pairwise restatement: random layers, 1 x 1 and odd sizes, equal keys, aliasing, 0 / 1
//                                layers, every argument error; fold_window against the fold of a layer padded with "none"
//   render_merge_driver window   a window never leaves the image whatever the camera and the rectangle (+-1e30, NaN, +-inf, 1 x 1 and
//                                odd images, rectangles touching 0 and 65536), and every pixel a particle of the rectangle's cells
//                                covers lies inside it
//   render_merge_driver window <gmin.x> <gmin.y> <h>   the coverage section on another cell grid (fp32 bit patterns, hex): the cameras
//                                as they are, and once more with their lengths scaled by h / 0.02
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "sphx_render_merge.hpp"
#include "sphx_render_window.hpp"

namespace {

int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            std::printf("FAILED: " __VA_ARGS__); \
            std::printf("\n");                \
            ++failures;                       \
        }                                     \
    } while (0)

constexpr uint32_t NONE = (uint32_t)SPHX_RENDER_NONE, BND = (uint32_t)SPHX_RENDER_BOUNDARY;

struct Layer {
    std::vector<uint32_t> key, owner;
    std::vector<uint8_t> rgba;
    bool with_rgba;
    Layer(size_t n, bool c) : key(n), owner(n), rgba(c ? 4 * n : 0), with_rgba(c) {}
    sphx_render_layer view() { return sphx_render_layer{key.data(), owner.data(), with_rgba ? rgba.data() : nullptr}; }
};

Layer random_layer(std::mt19937& g, size_t n, bool rgba, uint32_t tag) {
    Layer l(n, rgba);
    for (size_t p = 0; p < n; ++p) {
        const uint32_t kind = g() % 4u;
        l.owner[p] = kind == 0 ? NONE : kind == 1 ? BND : g() % 1000u;
        l.key[p] = kind >= 2 ? g() % 6u : 0u;  // (few values: equal keys are common)
        if (rgba)
            for (int k = 0; k < 4; ++k) l.rgba[4 * p + k] = (uint8_t)(tag * 16u + (g() & 15u));  // (the tag tells whose bytes arrived)
    }
    return l;
}

// the rule once more, two layers at a time and written down differently: class by comparison chain, decision by case
int cls(uint32_t o) { return o == NONE ? 0 : (o == BND ? 1 : 2); }
bool later_wins(uint32_t oa, uint32_t ka, uint32_t ob, uint32_t kb) {
    if (cls(ob) != cls(oa)) return cls(ob) > cls(oa);
    return cls(ob) == 2 && kb > ka;
}
Layer pairwise(std::vector<Layer>& ls, size_t n, bool rgba) {
    Layer acc(n, rgba);
    for (size_t p = 0; p < n; ++p) acc.owner[p] = NONE, acc.key[p] = 0;
    if (ls.empty()) return acc;
    acc = ls[0];
    for (size_t k = 1; k < ls.size(); ++k)
        for (size_t p = 0; p < n; ++p)
            if (later_wins(acc.owner[p], acc.key[p], ls[k].owner[p], ls[k].key[p])) {
                acc.owner[p] = ls[k].owner[p];
                acc.key[p] = ls[k].key[p];
                if (rgba) std::memcpy(&acc.rgba[4 * p], &ls[k].rgba[4 * p], 4);
            }
    return acc;
}
bool same(const Layer& a, const Layer& b) { return a.key == b.key && a.owner == b.owner && a.rgba == b.rgba; }

void check_merge() {
    std::mt19937 g(12345);
    const uint32_t sizes[][2] = {{1, 1}, {1, 7}, {5, 1}, {37, 23}, {3, 3}, {64, 2}};
    for (const auto& wh : sizes) {
        const size_t n = (size_t)wh[0] * wh[1];
        for (uint32_t nl = 0; nl <= 5; ++nl)
            for (int rgba = 0; rgba < 2; ++rgba) {
                if (nl == 0 && rgba) continue;
                std::vector<Layer> ls;
                for (uint32_t k = 0; k < nl; ++k) ls.push_back(random_layer(g, n, rgba, k));
                const Layer want = pairwise(ls, n, rgba);
                std::vector<sphx_render_layer> v;
                for (auto& l : ls) v.push_back(l.view());
                Layer got(n, rgba);
                sphx_render_layer o = got.view();
                const char* e = sphx_render_host::merge_error(wh[0], wh[1], v.data(), nl, &o);
                CHECK(!e, "%ux%u, %u layers: refused (%s)", wh[0], wh[1], nl, e ? e : "");
                sphx_render_host::merge(wh[0], wh[1], v.data(), nl, &o);
                CHECK(same(got, want), "%ux%u, %u layers, rgba %d: the fold differs from the pairwise restatement", wh[0], wh[1], nl, rgba);
                if (nl) {  // out aliases layers[0]
                    sphx_render_layer alias = v[0];
                    sphx_render_host::merge(wh[0], wh[1], v.data(), nl, &alias);
                    CHECK(same(ls[0], want), "%ux%u, %u layers: out aliasing layers[0] differs", wh[0], wh[1], nl);
                }
                if (nl == 1) CHECK(same(got, pairwise(ls, n, rgba)), "one layer is not returned as it is");
            }
    }
    // the order of two layers: fluid over boundary over none whichever comes first; equal keys keep the earlier; rgba follows the owner
    {
        Layer a(4, true), b(4, true);
        const uint32_t ao[4] = {7, BND, NONE, 7}, ak[4] = {5, 0, 0, 5}, bo[4] = {BND, NONE, 9, 8}, bk[4] = {0, 0, 1, 5};
        for (int p = 0; p < 4; ++p) {
            a.owner[p] = ao[p], a.key[p] = ak[p], b.owner[p] = bo[p], b.key[p] = bk[p];
            for (int k = 0; k < 4; ++k) a.rgba[4 * p + k] = 0xA0, b.rgba[4 * p + k] = 0xB0;
        }
        for (int order = 0; order < 2; ++order) {
            sphx_render_layer v[2] = {order ? b.view() : a.view(), order ? a.view() : b.view()};
            Layer got(4, true);
            sphx_render_layer o = got.view();
            sphx_render_host::merge(2, 2, v, 2, &o);
            const uint32_t wo[4] = {7, BND, 9, order ? 8u : 7u};
            const uint8_t wc[4] = {0xA0, 0xA0, 0xB0, (uint8_t)(order ? 0xB0 : 0xA0)};
            for (int p = 0; p < 4; ++p) CHECK(got.owner[p] == wo[p] && got.rgba[4 * p] == wc[p] && got.rgba[4 * p + 3] == wc[p], "two layers, order %d, pixel %d", order, p);
        }
    }
    // fold_window = the fold of the window padded with none
    for (int trial = 0; trial < 50; ++trial) {
        const uint32_t W = 1 + g() % 19u, H = 1 + g() % 13u;
        uint32_t x0 = g() % (W + 1), x1 = g() % (W + 1), y0 = g() % (H + 1), y1 = g() % (H + 1);
        if (x0 > x1) std::swap(x0, x1);
        if (y0 > y1) std::swap(y0, y1);
        const size_t n = (size_t)W * H, nw = (size_t)(x1 - x0) * (y1 - y0);
        Layer acc = random_layer(g, n, true, 1), win = random_layer(g, nw, true, 2), pad(n, true);
        for (size_t p = 0; p < n; ++p) pad.owner[p] = NONE, pad.key[p] = 0;
        for (uint32_t iy = y0; iy < y1; ++iy)
            for (uint32_t ix = x0; ix < x1; ++ix) {
                const size_t s = (size_t)(iy - y0) * (x1 - x0) + (ix - x0), d = (size_t)iy * W + ix;
                pad.owner[d] = win.owner[s], pad.key[d] = win.key[s];
                std::memcpy(&pad.rgba[4 * d], &win.rgba[4 * s], 4);
            }
        std::vector<Layer> two{acc, pad};
        const Layer want = pairwise(two, n, true);
        sphx_render_host::fold_window(acc.view(), W, win.view(), x0, x1, y0, y1);
        CHECK(same(acc, want), "fold_window %ux%u window [%u,%u)x[%u,%u)", W, H, x0, x1, y0, y1);
    }
    // every argument error
    {
        Layer a(4, true), o(4, true), nocol(4, false);
        sphx_render_layer la = a.view(), lo = o.view(), ln = nocol.view(), none{nullptr, nullptr, nullptr};
        sphx_render_layer nokey = la, noowner = la;
        nokey.key = nullptr, noowner.owner = nullptr;
        using sphx_render_host::merge_error;
        CHECK(merge_error(2, 2, &la, 1, nullptr), "out NULL accepted");
        CHECK(merge_error(2, 2, &la, 1, &none), "out requesting nothing accepted");
        CHECK(merge_error(2, 2, nullptr, 1, &lo), "layers NULL accepted");
        CHECK(merge_error(2, 2, &nokey, 1, &lo) && merge_error(2, 2, &noowner, 1, &lo), "a layer without key / owner accepted");
        CHECK(merge_error(2, 2, &ln, 1, &lo), "rgba requested, missing in a layer: accepted");
        CHECK(!merge_error(2, 2, &ln, 1, &ln), "no rgba anywhere refused");
        CHECK(merge_error(1u << 14, 1u << 14, &la, 1, &lo) && merge_error(0xFFFFFFFFu, 0xFFFFFFFFu, &la, 1, &lo), "width * height >= 2^28 accepted");
        CHECK(!merge_error((1u << 14) - 1u, 1u << 14, &la, 1, &ln), "width * height < 2^28 refused");
        CHECK(merge_error(2, 2, nullptr, 0, &lo), "n_layers == 0 with rgba accepted");
        CHECK(!merge_error(2, 2, nullptr, 0, &ln) && !merge_error(0, 0, nullptr, 0, &ln), "n_layers == 0 without rgba refused");
        sphx_render_host::merge(2, 2, nullptr, 0, &ln);
        for (int p = 0; p < 4; ++p) CHECK(nocol.owner[p] == NONE && nocol.key[p] == 0, "n_layers == 0 does not fill with none");
    }
}

// ---- the window ----------------------------------------------------------------------------------------------------------------------
uint32_t cell_coord(float v, float gmin, float cell_inv) {  // the grid's fp32 cell function
    const float c = (v - gmin) * cell_inv;
    if (!(c > 0.0f)) return 0;
    if (c >= 65535.0f) return 65535;
    return (uint32_t)c;
}

float from_bits(const char* hex) {
    const uint32_t u = (uint32_t)std::strtoul(hex, nullptr, 16);
    float f;
    std::memcpy(&f, &u, sizeof(f));
    return f;
}

struct Cam {
    uint32_t w, h;
    float cx, cy, ppu, r;
};

// nothing is lost: every pixel a particle covers (the contract's own fp32 test) lies in the window of every rectangle holding the
// particle's cell; particles far outside the domain land in the saturated cells of an outer rectangle
uint64_t check_coverage(const float gmin[2], float cell_inv, float particle_radius, const Cam* cams, size_t n_cams, uint32_t seed) {
    using namespace sphx;
    std::mt19937 g(seed);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    uint64_t covered = 0;
    for (size_t i = 0; i < n_cams; ++i) {
        const Cam& c = cams[i];
        sphx_render_view view;
        std::memset(&view, 0, sizeof(view));
        view.width = c.w, view.height = c.h, view.center[0] = c.cx, view.center[1] = c.cy, view.pixel_per_world_unit = c.ppu, view.radius = c.r;
        CHECK(!render_view_error(&view, 10.0f * particle_radius), "a good view is refused");
        const RenderCam v = render_make_cam(view, particle_radius);
        const float spanx = (float)c.w / c.ppu, spany = (float)c.h / c.ppu;
        for (int k = 0; k < 4000; ++k) {
            float px = c.cx + (u(g) - 0.5f) * spanx * 1.3f, py = c.cy + (u(g) - 0.5f) * spany * 1.3f;
            if (k % 50 == 0) px = -1e6f * u(g);  // far outside the domain: cell 0
            if (k % 50 == 1) py = 1e6f * u(g);   // ... cell 65535
            const uint32_t cx = cell_coord(px, gmin[0], cell_inv), cy = cell_coord(py, gmin[1], cell_inv);
            // rectangles holding the cell: a thin one with the cell at either edge, strips cut right at the cell, the cell alone
            const uint32_t rs[][4] = {{cx, cx + 1, cy, cy + 1}, {0, cx + 1, 0, 65536}, {cx, 65536, 0, 65536}, {0, 65536, 0, cy + 1}, {0, 65536, cy, 65536}};
            const RenderRect pr = render_pixel_rect(v, px, py);
            for (const auto& rc : rs) {
                const RenderWindow w = render_tile_window(v, rc[0], rc[1], rc[2], rc[3], gmin[0], gmin[1], cell_inv);
                for (uint32_t iy = pr.y0; iy < pr.y1; ++iy)
                    for (uint32_t ix = pr.x0; ix < pr.x1; ++ix)
                        if (render_covers(v, px, py, render_qx(v, ix), render_qy(v, iy))) {
                            ++covered;
                            CHECK(ix >= w.x0 && ix < w.x1 && iy >= w.y0 && iy < w.y1, "particle (%g, %g) of cell (%u, %u) covers pixel (%u, %u) outside the window [%u,%u)x[%u,%u)",
                                  px, py, cx, cy, ix, iy, w.x0, w.x1, w.y0, w.y1);
                        }
            }
        }
    }
    return covered;
}

const Cam CAMS[] = {{320, 240, 0.95f, 0.7f, 145.45454f, 0.015f}, {320, 240, 0.95f, 0.7f, 145.45454f, 0.005f}, {37, 23, 0.4f, 0.3f, 30.0f, 0.02f},
                    {160, 120, 0.35f, 0.5f, 2000.0f, 0.02f},    {1, 1, 0.34f, 0.5f, 40.0f, 0.02f},          {64, 48, 0.95f, 0.7f, 20.0f, 0.0375f},
                    {200, 100, -120.0f, 0.5f, 4.0f, 0.02f},     {101, 99, 1300.0f, 1250.0f, 0.5f, 0.02f}};
constexpr size_t N_CAMS = sizeof(CAMS) / sizeof(CAMS[0]);

// the coverage section on the cell grid (gmin, h) of the command line: the cameras as they are (cells of another size under the same
// discs), then with every length scaled by h / 0.02 (the same picture in cells), the particle radius h / 4 as at smoothing factor 2
void check_window_at(const float gmin[2], float h) {
    const float cell_inv = 1.0f / h, s = h / 0.02f;
    uint64_t covered = check_coverage(gmin, cell_inv, 0.005f, CAMS, N_CAMS, 777);
    Cam scaled_cams[N_CAMS];
    for (size_t i = 0; i < N_CAMS; ++i) scaled_cams[i] = Cam{CAMS[i].w, CAMS[i].h, CAMS[i].cx * s, CAMS[i].cy * s, CAMS[i].ppu / s, CAMS[i].r * s};
    covered += check_coverage(gmin, cell_inv, 0.25f * h, scaled_cams, N_CAMS, 778);
    CHECK(covered > 200000, "the scenes cover too few pixels (%llu)", (unsigned long long)covered);
    std::printf("window: %llu covered pixels inside their windows at grid_min (%g, %g), h %.9g\n", (unsigned long long)covered, gmin[0], gmin[1], h);
}

void check_window() {
    using namespace sphx;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float hostile[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.95f, 1e-38f, 1e30f, -1e30f, 3.4e38f, -3.4e38f, inf, -inf, nan, 65536.0f, 1e9f};
    const uint32_t sizes[][2] = {{1, 1}, {1, 777}, {333, 1}, {37, 23}, {320, 240}, {1u << 20, 200}};
    const uint32_t rects[][4] = {{0, 65536, 0, 65536}, {0, 5017, 0, 65536}, {5017, 65536, 0, 65536}, {5005, 5030, 5010, 5040}, {0, 1, 0, 1},
                                 {65535, 65536, 65535, 65536}, {5017, 5017, 0, 65536}, {7, 3, 0, 65536}, {0, 65536, 5030, 5031}};
    const float gmin = -100.0f, cell_inv = 1.0f / 0.02f;
    uint64_t n = 0;
    for (const auto& wh : sizes)
        for (float cx : hostile)
            for (float cy : {0.7f, cx})
                for (float ppu : {145.45454f, 1e-3f, 1e7f, 1e30f, inf, nan, 0.0f, -5.0f})
                    for (float r : {0.005f, 0.02f, 0.0f, 1e30f, inf, nan})
                        for (const auto& rc : rects) {
                            RenderCam v;
                            v.cx = cx, v.cy = cy, v.ppu = ppu, v.inv = 1.0f / ppu, v.r = r, v.r2 = r * r, v.width = wh[0], v.height = wh[1];
                            const RenderWindow w = render_tile_window(v, rc[0], rc[1], rc[2], rc[3], gmin, gmin, cell_inv);
                            CHECK(w.x0 <= w.x1 && w.x1 <= wh[0] && w.y0 <= w.y1 && w.y1 <= wh[1], "window [%u,%u)x[%u,%u) leaves the %ux%u image (centre %g %g ppu %g r %g)",
                                  w.x0, w.x1, w.y0, w.y1, wh[0], wh[1], cx, cy, ppu, r);
                            ++n;
                        }
    // the same with a hostile grid
    for (float g0 : hostile)
        for (float ci : {50.0f, 1e-30f, 1e30f, inf, nan, 0.0f, -1.0f}) {
            RenderCam v;
            v.cx = 0.95f, v.cy = 0.7f, v.ppu = 145.0f, v.inv = 1.0f / 145.0f, v.r = 0.015f, v.r2 = v.r * v.r, v.width = 37, v.height = 23;
            const RenderWindow w = render_tile_window(v, 5000, 5020, 0, 65536, g0, g0, ci);
            CHECK(w.x0 <= w.x1 && w.x1 <= 37 && w.y0 <= w.y1 && w.y1 <= 23, "hostile grid: window leaves the image");
            ++n;
        }
    std::printf("window: %llu windows inside their images\n", (unsigned long long)n);

    const float gmin2[2] = {gmin, gmin};
    const uint64_t covered = check_coverage(gmin2, cell_inv, 0.005f, CAMS, N_CAMS, 777);
    CHECK(covered > 100000, "the scenes cover too few pixels (%llu)", (unsigned long long)covered);
    std::printf("window: %llu covered pixels inside their windows\n", (unsigned long long)covered);
    // a window is not the whole image where it need not be: a strip's window ends near the cut
    {
        sphx_render_view view;
        std::memset(&view, 0, sizeof(view));
        view.width = 320, view.height = 240, view.center[0] = 0.95f, view.center[1] = 0.7f, view.pixel_per_world_unit = 145.45454f, view.radius = 0.015f;
        const RenderCam v = render_make_cam(view, 0.005f);
        const RenderWindow a = render_tile_window(v, 0, 5017, 0, 65536, gmin, gmin, cell_inv), b = render_tile_window(v, 5017, 65536, 0, 65536, gmin, gmin, cell_inv);
        // cell 5017 starts at x = 0.34: pixel column (0.34 - 0.95) * 145.45 + 160 = 71.3; radius 2.2 pixels, one cell 2.9 pixels
        CHECK(a.x0 == 0 && a.x1 >= 74 && a.x1 <= 82 && b.x0 >= 62 && b.x0 <= 69 && b.x1 == 320, "strip windows [%u,%u) and [%u,%u)", a.x0, a.x1, b.x0, b.x1);
        CHECK(a.y0 == 0 && a.y1 == 240 && b.y0 == 0 && b.y1 == 240, "strip windows do not span the rows");
    }
}

}  // namespace

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "merge")
        check_merge();
    else if (what == "window" && argc >= 5) {
        const float gmin[2] = {from_bits(argv[2]), from_bits(argv[3])};
        check_window_at(gmin, from_bits(argv[4]));
    } else if (what == "window")
        check_window();
    else {
        std::printf("usage: render_merge_driver merge|window [gmin.x gmin.y h as fp32 bit patterns]\n");
        return 2;
    }
    if (!failures) std::printf("ok %s\n", what.c_str());
    return failures ? 1 : 0;
}
