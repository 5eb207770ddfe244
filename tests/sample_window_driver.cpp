// Stand-alone driver of yasph2d_amd/csrc/sphx_sample_window.hpp (no GPU, no HIP): the bisection's index rectangle of a tile in a
// sampling lattice against the brute-force set {(ix, iy) : cell in rect}, and the fold of the ranks' parts.  Built by
// tests/test_sample_multi_host.py with -ffp-contract=off and -fsanitize=address,undefined and run directly.
//   sample_window_driver check        -> "ok <cases>" after a few hundred seeded lattices and rectangles
//   sample_window_driver dump <k>     -> k of those cases, one per line, floats as their bit patterns (the Python side restates them)
//   sample_window_driver merge        -> "ok <cases>": the fold against a restatement, aliasing out = parts[0] included
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "sphx_sample_window.hpp"

namespace sh = sphx_sample_host;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t below(uint32_t n) { return n ? (uint32_t)(rnd() % n) : 0u; }
static float unit() { return (float)(rnd() >> 40) * (1.0f / 16777216.0f); }
static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

struct Case {
    float x0, y0, dx, dy;
    uint32_t nx, ny;
    float gx, gy, cell_inv;
    uint32_t cx0, cx1, cy0, cy1;
};

// one axis of a lattice: origin, spacing, count.  kind picks the regime the issue lists.
static void axis(int kind, float gmin, float cell, float& o, float& d, uint32_t& n) {
    const float span = 65536.0f * cell;  // the domain along the axis is [gmin, gmin + span)
    n = 1u + below(200);
    switch (kind % 8) {
        case 0: d = cell * (0.05f + 0.9f * unit()); o = gmin + span * unit() * 0.01f; break;          // below one cell
        case 1: d = cell; o = gmin + cell * (float)below(1000) + cell * unit(); break;                   // exactly one cell
        case 2: d = cell * (1.0f + 20.0f * unit()); o = gmin + span * unit() * 0.01f; break;             // above one cell
        case 3: n = 1; d = cell * (0.1f + 3.0f * unit()); o = gmin + span * unit(); break;               // a single index
        case 4: d = cell * (0.3f + 2.0f * unit()); o = gmin - cell * (float)(1 + below(50)) - cell * unit(); break;  // starts below the domain
        case 5: d = cell * (0.3f + 2.0f * unit()); o = gmin + span - cell * (float)below(60) + cell * unit(); break;  // runs out above it
        case 6: d = 1.0e38f * (0.5f + 2.0f * unit()); o = gmin + cell * (float)below(100); break;       // (float)i * d reaches +inf
        default: d = span / (float)n * (0.5f + unit()); o = gmin - span * 0.1f * unit(); break;          // spans the whole domain
    }
}

// cuts of a rectangle along one axis, chosen around the cells the lattice really visits so that the window is rarely trivial
static void cuts(float o, float d, uint32_t n, float gmin, float cell_inv, uint32_t& c0, uint32_t& c1) {
    const uint32_t lo = sh::lattice_cell(o, d, 0, gmin, cell_inv), hi = sh::lattice_cell(o, d, n - 1, gmin, cell_inv);
    auto pick = [&]() -> uint32_t {
        switch (below(6)) {
            case 0: return 0u;
            case 1: return 65536u;
            case 2: return lo;
            case 3: return hi + (hi < 65536u ? 1u : 0u);
            default: return lo + below(hi - lo + 2u);
        }
    };
    uint32_t a = pick(), b = pick();
    if (a > b) std::swap(a, b);
    if (a == b) {  // (a rectangle is not empty)
        if (a < 65536u)
            b = a + 1u;
        else
            a = b - 1u;
    }
    c0 = a, c1 = b;
}

static Case make_case(uint32_t k) {
    Case c;
    const bool odd_grid = (k % 5) == 4;
    const float cell = odd_grid ? 0.013f + 0.1f * unit() : 0.02f;
    c.gx = odd_grid ? -3.0f - 50.0f * unit() : -100.0f;
    c.gy = odd_grid ? 7.0f * unit() : -100.0f;
    c.cell_inv = 1.0f / cell;
    axis((int)k, c.gx, cell, c.x0, c.dx, c.nx);
    axis((int)(k / 8 + k), c.gy, cell, c.y0, c.dy, c.ny);
    cuts(c.x0, c.dx, c.nx, c.gx, c.cell_inv, c.cx0, c.cx1);
    cuts(c.y0, c.dy, c.ny, c.gy, c.cell_inv, c.cy0, c.cy1);
    return c;
}

static int fail(const char* what, uint32_t k) {
    std::printf("FAILED case %u: %s\n", k, what);
    return 1;
}

// the brute-force set of one case against the window; returns non-zero on a mismatch
static int check_case(const Case& c, uint32_t k, const sh::Window& w) {
    if (w.ix0 > w.ix1 || w.ix1 > c.nx || w.iy0 > w.iy1 || w.iy1 > c.ny) return fail("the window leaves the lattice", k);
    uint64_t members = 0;
    for (uint32_t iy = 0; iy < c.ny; ++iy)
        for (uint32_t ix = 0; ix < c.nx; ++ix) {
            const uint32_t cx = sh::lattice_cell(c.x0, c.dx, ix, c.gx, c.cell_inv), cy = sh::lattice_cell(c.y0, c.dy, iy, c.gy, c.cell_inv);
            const bool in_rect = cx >= c.cx0 && cx < c.cx1 && cy >= c.cy0 && cy < c.cy1;
            const bool in_win = ix >= w.ix0 && ix < w.ix1 && iy >= w.iy0 && iy < w.iy1;
            if (in_rect != in_win) return fail(in_rect ? "a point of the rectangle is outside the window" : "the window holds a point of another rectangle", k);
            members += in_rect;
        }
    if (members != w.points()) return fail("the window's size is not the set's", k);
    return 0;
}

static int run_check(uint32_t n_cases, uint32_t dump) {
    uint32_t nonempty = 0, whole = 0, inf_cases = 0;
    for (uint32_t k = 0; k < n_cases; ++k) {
        const Case c = make_case(k);
        const sh::Window w = sh::lattice_window(c.x0, c.y0, c.dx, c.dy, c.nx, c.ny, c.gx, c.gy, c.cell_inv, c.cx0, c.cx1, c.cy0, c.cy1);
        if (check_case(c, k, w)) return 1;
        nonempty += w.points() != 0;
        whole += w.points() == (uint64_t)c.nx * c.ny;
        const float last = (float)(c.nx - 1) * c.dx;
        inf_cases += last == std::numeric_limits<float>::infinity();
        // a partition: the windows of complementary strips are disjoint and cover the lattice
        const sh::Window a = sh::lattice_window(c.x0, c.y0, c.dx, c.dy, c.nx, c.ny, c.gx, c.gy, c.cell_inv, 0, c.cx0, 0, 65536);
        const sh::Window b = sh::lattice_window(c.x0, c.y0, c.dx, c.dy, c.nx, c.ny, c.gx, c.gy, c.cell_inv, c.cx0, c.cx1, 0, 65536);
        const sh::Window d = sh::lattice_window(c.x0, c.y0, c.dx, c.dy, c.nx, c.ny, c.gx, c.gy, c.cell_inv, c.cx1, 65536, 0, 65536);
        if (a.points() + b.points() + d.points() != (uint64_t)c.nx * c.ny) return fail("three strips do not partition the lattice", k);
        if (k < dump)
            std::printf("%08x %08x %08x %08x %u %u %08x %08x %08x %u %u %u %u %u %u %u %u\n", bits(c.x0), bits(c.y0), bits(c.dx), bits(c.dy), c.nx, c.ny, bits(c.gx),
                        bits(c.gy), bits(c.cell_inv), c.cx0, c.cx1, c.cy0, c.cy1, w.ix0, w.ix1, w.iy0, w.iy1);
    }
    if (!dump) {
        if (nonempty < n_cases / 4 || whole == n_cases || !inf_cases) return fail("the cases do not exercise the window (empty, whole or no infinity)", n_cases);
        std::printf("ok %u\n", n_cases);
    }
    return 0;
}

static int run_merge() {
    uint32_t cases = 0;
    for (uint32_t round = 0; round < 60; ++round) {
        const uint32_t m = round == 0 ? 0u : 1u + below(97), n_parts = round % 7 == 1 ? 0u : 1u + below(4);
        std::vector<std::vector<uint32_t>> den(n_parts), fra(n_parts), vel(n_parts), cnt(n_parts);
        std::vector<std::vector<int32_t>> tile(n_parts);
        for (uint32_t p = 0; p < n_parts; ++p) {
            den[p].resize(m), fra[p].resize(m), vel[p].resize(2 * (size_t)m), cnt[p].resize(m), tile[p].resize(m);
            for (uint32_t k = 0; k < m; ++k) {
                const bool on = below(3) != 0;
                tile[p][k] = on ? (int32_t)below(5) : -1;  // (tiles repeat across parts: "two parts answering one point")
                den[p][k] = on ? (uint32_t)rnd() : 0u, fra[p][k] = on ? (uint32_t)rnd() : 0u, cnt[p][k] = on ? below(80) : 0u;
                vel[p][2 * (size_t)k] = on ? (uint32_t)rnd() : 0u, vel[p][2 * (size_t)k + 1] = on ? (uint32_t)rnd() : 0u;
            }
        }
        // the restatement
        std::vector<uint32_t> wd(m, 0u), wf(m, 0u), wv(2 * (size_t)m, 0u), wc(m, 0u);
        std::vector<int32_t> wt(m, -1);
        for (uint32_t k = 0; k < m; ++k)
            for (uint32_t p = 0; p < n_parts; ++p)
                if (tile[p][k] >= 0 && (wt[k] < 0 || tile[p][k] < wt[k]))
                    wt[k] = tile[p][k], wd[k] = den[p][k], wf[k] = fra[p][k], wc[k] = cnt[p][k], wv[2 * (size_t)k] = vel[p][2 * (size_t)k],
                    wv[2 * (size_t)k + 1] = vel[p][2 * (size_t)k + 1];
        std::vector<sh::Part> parts(n_parts);
        for (uint32_t p = 0; p < n_parts; ++p) parts[p] = sh::Part{den[p].data(), fra[p].data(), vel[p].data(), cnt[p].data(), tile[p].data()};
        const bool alias = n_parts && round % 2 == 0;
        std::vector<uint32_t> od(m, 7u), of(m, 7u), ov(2 * (size_t)m, 7u), oc(m, 7u);
        std::vector<int32_t> ot(m, 7);
        const sh::Acc acc = alias ? sh::Acc{den[0].data(), fra[0].data(), vel[0].data(), cnt[0].data(), tile[0].data()}
                                  : sh::Acc{od.data(), of.data(), ov.data(), oc.data(), ot.data()};
        sh::merge(m, parts.data(), n_parts, acc);
        if (m && (std::memcmp(acc.density, wd.data(), (size_t)m * 4) || std::memcmp(acc.fraction, wf.data(), (size_t)m * 4) || std::memcmp(acc.velocity, wv.data(), (size_t)m * 8) ||
                  std::memcmp(acc.count, wc.data(), (size_t)m * 4) || std::memcmp(acc.tile, wt.data(), (size_t)m * 4)))  // (m == 0: the vectors have no storage)
            return fail("the fold differs from its restatement", round);
        // a subset of the outputs leaves the others alone
        std::vector<uint32_t> only(m, 9u);
        if (!alias && m) {
            sh::merge(m, parts.data(), n_parts, sh::Acc{nullptr, only.data(), nullptr, nullptr, nullptr});
            if (std::memcmp(only.data(), wf.data(), (size_t)m * 4)) return fail("the fraction-only fold differs", round);
        }
        cases += 1;
    }
    std::printf("ok %u\n", cases);
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "check";
    if (mode == "check") return run_check(480, 0);
    if (mode == "dump") return run_check(480, argc > 2 ? (uint32_t)std::atoi(argv[2]) : 40u);
    if (mode == "merge") return run_merge();
    std::printf("unknown mode\n");
    return 2;
}
