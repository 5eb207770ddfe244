// Stand-alone driver for the tiled gauge headers (yasph2d_amd/csrc/sphx_gauge_window.hpp, sphx_gauge_merge.hpp): plain C++, compiled by
// tests/test_gauge_multi_host.py with the address and undefined-behaviour sanitizers (any report aborts the program) and without
// value-changing floating-point options.
//   gauge_merge_driver self
//     The headers' own grid of cases: the bisection interval against the brute-force owned set (rays of every direction, zero steps,
//     steps that overflow, rays that leave the domain; strips and 2 x 2 rectangles), and the fold of make_part over every split of seeded
//     value arrays into up to five intervals against reduce_one.  Prints "ok <cases>"; returns 1 on the first difference.
//   gauge_merge_driver window IN OUT
//     IN:  float gmin_x, gmin_y, cell_inv, uint32 n_rects, n_gauges, n_rects x {x0, x1, y0, y1}, n_gauges x sphx_gauge.
//     OUT: [n_rects][n_gauges] x {lo, count} as gauge_interval found them.
//   gauge_merge_driver fold IN OUT
//     IN:  uint32 n_gauges, float iso, uint32 n_parts, n_gauges x sphx_gauge, [n_parts][n_gauges] x sphx_gauge_part.
//     OUT: n_gauges x sphx_gauge_rec as sphx_gauge_host::merge wrote them (untouched 0xAB bytes on a refusal).  Prints "rc 0", or "rc 1
//     <message>".
// The arrays are heap blocks of exactly the needed size, so a read or write behind any is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sphx_gauge_merge.hpp"

namespace gh = sphx_gauge_host;

static bool read_all(const char* path, std::vector<unsigned char>& out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    unsigned char buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + n);
    std::fclose(f);
    return true;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

struct Rect {
    uint32_t x0, x1, y0, y1;
};

static int self_window(uint64_t& cases) {
    struct Grid {
        float gx, gy, h;
    };
    const Grid grids[] = {{-100.0f, -100.0f, 0.02f}, {-3.0f, -7.5f, 0.01f}, {-1.0f, -1.0f, 0.0025000002f}, {-500.0f, -500.0f, 0.18033393f}};
    for (const Grid& G : grids) {
        const float inv = 1.0f / G.h;
        const uint32_t cx = sphx_sample_host::cell_coord(0.5f, G.gx, inv), cy = sphx_sample_host::cell_coord(0.3f, G.gy, inv);
        const Rect rects[] = {{0, cx, 0, 65536},       {cx, 65536, 0, 65536},                               // 2 strips
                              {0, cx - 7, 0, 65536},   {cx - 7, cx + 9, 0, 65536}, {cx + 9, 65536, 0, 65536},  // 3 strips
                              {0, cx, 0, cy},          {0, cx, cy, 65536},         {cx, 65536, 0, cy + 3},  {cx, 65536, cy + 3, 65536},  // 2 x 2
                              {0, 65536, 0, cy},       {0, 65536, cy, 65536}};                             // 2 strips along y
        const float steps[] = {0.0f, -0.0f, G.h * 0.37f, -G.h * 0.37f, G.h * 3.1f, -G.h * 2.9f, 1e-30f, 1e30f, -1e30f, 3e38f, -3e38f, G.h};
        for (float dx : steps)
            for (float dy : steps)
                for (int o = 0; o < 4; ++o) {
                    const float x0 = o == 0 ? 0.5f : o == 1 ? 0.5f - 40.0f * G.h : o == 2 ? G.gx - 5.0f * G.h : 3e38f;
                    const float y0 = o == 0 ? 0.3f : o == 1 ? 0.3f + 33.0f * G.h : o == 2 ? G.gy + 70000.0f * G.h : -3e38f;
                    const uint32_t n = 1u + rnd() % 300u;
                    std::vector<uint32_t> owners(n, 0u);
                    for (const Rect& r : rects) {
                        const gh::Interval iv = gh::gauge_interval(x0, y0, dx, dy, n, G.gx, G.gy, inv, r.x0, r.x1, r.y0, r.y1);
                        for (uint32_t k = 0; k < n; ++k) {
                            const bool own = gh::sample_owned(x0, y0, dx, dy, k, G.gx, G.gy, inv, r.x0, r.x1, r.y0, r.y1);
                            const bool in = k >= iv.lo && k < iv.lo + iv.count;
                            if (own != in) {
                                std::printf("window: sample %u of (%g, %g, %g, %g, %u) in rect (%u, %u, %u, %u): owned %d, interval [%u, +%u)\n", k, x0, y0, dx,
                                            dy, n, r.x0, r.x1, r.y0, r.y1, (int)own, iv.lo, iv.count);
                                return 1;
                            }
                            owners[k] += own ? 1u : 0u;
                        }
                        cases += 1;
                    }
                    for (uint32_t k = 0; k < n; ++k)
                        if (owners[k] != 4u) {  // (the rectangles above are four tilings of the cell domain)
                            std::printf("window: sample %u is owned %u times over four tilings\n", k, owners[k]);
                            return 1;
                        }
                }
    }
    return 0;
}

static int self_fold(uint64_t& cases) {
    for (uint32_t trial = 0; trial < 600u; ++trial) {
        const uint32_t n = 1u + (trial < 200u ? trial : rnd() % 200u);
        float* f = (float*)std::malloc((size_t)n * 4);
        const uint32_t mode = trial % 5u;  // 0: a profile, 1: noise, 2: nothing inside, 3: everything inside, 4: NaNs
        for (uint32_t k = 0; k < n; ++k) {
            const float u = (float)(rnd() % 1000u) / 1000.0f;
            f[k] = mode == 0 ? 1.1f - (float)k / (float)n + 0.1f * u : mode == 1 ? u : mode == 2 ? 0.4f * u : mode == 3 ? 0.5f + u : (rnd() % 3u ? u : gh::qnan_value());
        }
        const sphx_gauge g{0.1f, 0.2f, 0.003f, -0.007f, n, {0u, 0u, 0u}};
        const gh::Words want = gh::reduce_one(g, f, 0.5f);
        const uint32_t last = want.w[1];
        for (uint32_t np = 1; np <= 5u; ++np)
            for (uint32_t rep = 0; rep < 6u; ++rep) {
                // cuts: random, but with `last + 1` (and `last`) forced into them on some repeats, so that last ends an interval
                std::vector<uint32_t> cuts(np + 1u, 0u);
                cuts[np] = n;
                for (uint32_t c = 1; c < np; ++c) cuts[c] = rnd() % (n + 1u);
                if (np > 1u && last != SPHX_GAUGE_NONE && rep % 3u == 1u) cuts[1 + rnd() % (np - 1u)] = last + 1u;
                if (np > 2u && last != SPHX_GAUGE_NONE && rep % 3u == 2u) cuts[1] = last, cuts[2] = last + 1u;
                for (uint32_t a = 1; a < np; ++a)  // ascending (equal cuts: empty parts)
                    for (uint32_t b = a + 1u; b < np; ++b)
                        if (cuts[b] < cuts[a]) std::swap(cuts[a], cuts[b]);
                sphx_gauge_part* parts = (sphx_gauge_part*)std::malloc((size_t)np * sizeof(sphx_gauge_part));
                for (uint32_t p = 0; p < np; ++p) parts[(p + rep) % np] = gh::make_part(f, gh::Interval{cuts[p], cuts[p + 1u] - cuts[p]}, 0.5f);  // (rotated: any order)
                gh::Words got;
                std::memset(&got, 0xAB, sizeof(got));
                const char* bad = gh::fold(g, 0.5f, parts, np, 1, &got);
                if (bad || std::memcmp(&got, &want, sizeof(got))) {
                    std::printf("fold: trial %u, n %u, %u parts, repeat %u: %s\n", trial, n, np, rep, bad ? bad : "the record differs from reduce_one");
                    return 1;
                }
                // refusals: a part moved, shortened or lengthened never gives a record
                if (n > 1u) {
                    sphx_gauge_part& q = parts[rnd() % np];
                    const sphx_gauge_part keep = q;
                    const uint32_t how = rep % 3u;
                    if (how == 0u) q.count += 1u;
                    else if (how == 1u && q.count) q.count -= 1u, q.inside = q.inside > q.count ? q.count : q.inside;
                    else q.lo += 1u;
                    const bool changed = std::memcmp(&q, &keep, sizeof(q)) != 0 && (keep.count != 0u || how == 0u);
                    gh::Words none;
                    std::memset(&none, 0xAB, sizeof(none));
                    const char* refused = gh::fold(g, 0.5f, parts, np, 1, &none);
                    if (changed && !refused) {
                        std::printf("fold: trial %u: a part with a wrong %s was folded\n", trial, how == 2u ? "lo" : "count");
                        return 1;
                    }
                }
                std::free(parts);
                cases += 1;
            }
        std::free(f);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "self")) {
        uint64_t cases = 0;
        if (self_window(cases) || self_fold(cases)) return 1;
        std::printf("ok %llu\n", (unsigned long long)cases);
        return 0;
    }
    if (argc != 4) return 2;
    std::vector<unsigned char> in;
    if (!read_all(argv[2], in)) return 2;
    if (!std::strcmp(argv[1], "window")) {
        if (in.size() < 20) return 2;
        float gm[3];
        uint32_t cnt[2];
        std::memcpy(gm, in.data(), 12);
        std::memcpy(cnt, in.data() + 12, 8);
        const uint32_t n_rects = cnt[0], n_gauges = cnt[1];
        if (n_rects > 4096u || n_gauges > 65536u || in.size() != 20 + (size_t)n_rects * 16 + (size_t)n_gauges * 32) return 2;
        Rect* rects = (Rect*)std::malloc((size_t)n_rects * sizeof(Rect) + 1);
        sphx_gauge* gauges = (sphx_gauge*)std::malloc((size_t)n_gauges * sizeof(sphx_gauge) + 1);
        std::memcpy(rects, in.data() + 20, (size_t)n_rects * 16);
        std::memcpy(gauges, in.data() + 20 + (size_t)n_rects * 16, (size_t)n_gauges * 32);
        FILE* f = std::fopen(argv[3], "wb");
        if (!f) return 2;
        for (uint32_t r = 0; r < n_rects; ++r)
            for (uint32_t k = 0; k < n_gauges; ++k) {
                const sphx_gauge& g = gauges[k];
                const gh::Interval iv = gh::gauge_interval(g.x0, g.y0, g.dx, g.dy, g.n, gm[0], gm[1], gm[2], rects[r].x0, rects[r].x1, rects[r].y0, rects[r].y1);
                std::fwrite(&iv, sizeof(iv), 1, f);
            }
        std::fclose(f);
        std::free(rects);
        std::free(gauges);
        return 0;
    }
    if (!std::strcmp(argv[1], "fold")) {
        if (in.size() < 12) return 2;
        uint32_t n_gauges, n_parts;
        float iso;
        std::memcpy(&n_gauges, in.data(), 4);
        std::memcpy(&iso, in.data() + 4, 4);
        std::memcpy(&n_parts, in.data() + 8, 4);
        if (n_gauges > 4096u || n_parts > 4096u || in.size() != 12 + (size_t)n_gauges * 32 + (size_t)n_parts * n_gauges * 32) return 2;
        sphx_gauge* gauges = (sphx_gauge*)std::malloc((size_t)n_gauges * 32 + 1);
        sphx_gauge_part* parts = (sphx_gauge_part*)std::malloc((size_t)n_parts * n_gauges * 32 + 1);
        sphx_gauge_rec* out = (sphx_gauge_rec*)std::malloc((size_t)n_gauges * 32 + 1);
        std::memcpy(gauges, in.data() + 12, (size_t)n_gauges * 32);
        std::memcpy(parts, in.data() + 12 + (size_t)n_gauges * 32, (size_t)n_parts * n_gauges * 32);
        std::memset(out, 0xAB, (size_t)n_gauges * 32);
        const char* bad = gh::merge(gauges, n_gauges, iso, parts, n_parts, out);
        std::printf("rc %d %s\n", bad ? 1 : 0, bad ? bad : "");
        FILE* f = std::fopen(argv[3], "wb");
        if (!f) return 2;
        std::fwrite(out, 32, n_gauges, f);
        std::fclose(f);
        std::free(gauges);
        std::free(parts);
        std::free(out);
        return 0;
    }
    return 2;
}
