// Host driver of tests/test_block_mapping.py: the XCD block mapping of the kernels (yasph2d_amd/csrc/sphx_xcd.hpp), compiled as
// plain C++.  Each command checks one property and prints "ok <cases>" or "FAIL ..." lines (at most a few), exit status 0 / 1.
//   perm_exhaustive      every grid 8 per, per in [1, 4096], every shift of the clamped range, both directions: a bijection
//   perm_sampled         the same for sampled per in (4096, 65536] (65 536: the 128 M particle grid)
//   scatter              the scatter's packed argument and derived shift; its grids (1 024-particle blocks) are bijections too
//   eighths              shift s with per < 2^s is the contiguous-eighths map (shift 0), e.g. shift 7 below 128 blocks per XCD
//   clamp v...           prints xcd_shift_clamp(v) for each v
//   map grid rev shift   prints the map of every block of one grid
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sphx_xcd.hpp"

using namespace sphx;

static int fails = 0;
static long long cases = 0;
static std::vector<uint32_t> seen;
static uint32_t stamp = 0;

static void fail_msg(const char* what, uint32_t grid, uint32_t rev, uint32_t shift, uint32_t block, uint32_t v) {
    if (fails++ < 8) std::printf("FAIL %s grid %u rev %u shift %u block %u -> %u\n", what, grid, rev, shift, block, v);
}

// every block lands in [0, grid) and no two on the same particle block
static void check_perm(uint32_t grid, uint32_t rev, uint32_t shift) {
    if (seen.size() < grid) seen.assign(grid, 0u);
    if (++stamp == 0) {
        std::fill(seen.begin(), seen.end(), 0u);
        stamp = 1;
    }
    ++cases;
    for (uint32_t b = 0; b < grid; ++b) {
        const uint32_t v = xcd_map(b, grid, rev, shift);
        if (v >= grid) return fail_msg("out of range", grid, rev, shift, b, v);
        if (seen[v] == stamp) return fail_msg("hit twice", grid, rev, shift, b, v);
        seen[v] = stamp;
    }
}

static void perm_all_shifts(uint32_t per) {
    for (int s = 0; s <= XCD_SHIFT_MAX; ++s)
        for (uint32_t rev = 0; rev < 2; ++rev) check_perm(8u * per, rev, (uint32_t)s);
}

static int done() {
    if (fails) return 1;
    std::printf("ok %lld\n", cases);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* cmd = argv[1];
    if (!std::strcmp(cmd, "perm_exhaustive")) {
        for (uint32_t per = 1; per <= 4096; ++per) perm_all_shifts(per);
        return done();
    }
    if (!std::strcmp(cmd, "perm_sampled")) {
        // powers of two and their neighbours, multiples of the default chunk +- 1, and a fixed pseudo-random sample
        std::vector<uint32_t> pers;
        for (uint32_t p = 8192; p <= 65536; p *= 2) pers.insert(pers.end(), {p - 1, p, p + 1});
        for (uint32_t k = 33; k <= 512; k += 53) pers.insert(pers.end(), {128 * k - 1, 128 * k, 128 * k + 1});
        uint32_t x = 12345u;
        for (int i = 0; i < 24; ++i) {
            x = x * 1664525u + 1013904223u;
            pers.push_back(4097u + (x >> 8) % (65536u - 4096u));
        }
        pers.push_back(65536u);
        for (uint32_t per : pers)
            if (per > 4096u && per <= 65536u) perm_all_shifts(per);
        return done();
    }
    if (!std::strcmp(cmd, "scatter")) {
        for (int s = 0; s <= XCD_SHIFT_MAX; ++s) {
            const uint32_t d = xcd_scatter_shift((uint32_t)s);
            // a chunk of the scatter (2^d blocks of 1 024 particles) covers a chunk of the 256-particle kernels (2^s blocks)
            if (s >= 2 && (1024ull << d) != (256ull << s)) fail_msg("derived shift", 0, 0, (uint32_t)s, 0, d);
            if (s < 2 && d != 0u) fail_msg("derived shift", 0, 0, (uint32_t)s, 0, d);
            for (uint32_t rev = 0; rev < 2; ++rev) {
                const uint32_t p = xcd_scatter_pack(rev, (uint32_t)s);
                if (xcd_packed_rev(p) != rev || xcd_packed_shift(p) != d) fail_msg("scatter packing", 0, rev, (uint32_t)s, 0, p);
                const uint32_t q = xcd_pack(rev, (uint32_t)s);
                if (xcd_packed_rev(q) != rev || xcd_packed_shift(q) != (uint32_t)s) fail_msg("packing", 0, rev, (uint32_t)s, 0, q);
            }
            // the scatter's grid: ceil(n / 1024) rounded up to a multiple of 8 (build_grid), for n over the context sizes
            for (uint64_t n = 1; n < (1ull << 28); n = n * 3 / 2 + 1) {
                const uint32_t grid = (uint32_t)(((n + 1023) / 1024 + 7) & ~7ull);
                for (uint32_t rev = 0; rev < 2; ++rev) {
                    const uint32_t p = xcd_scatter_pack(rev, (uint32_t)s);
                    check_perm(grid, xcd_packed_rev(p), xcd_packed_shift(p));
                }
            }
        }
        return done();
    }
    if (!std::strcmp(cmd, "eighths")) {
        for (uint32_t s = 1; s <= (uint32_t)XCD_SHIFT_MAX; ++s)
            for (uint32_t per = 1; per < (1u << s) && per <= 512u; ++per)
                for (uint32_t rev = 0; rev < 2; ++rev) {
                    ++cases;
                    for (uint32_t b = 0; b < 8u * per; ++b) {
                        const uint32_t x = b & 7u, q = rev ? per - 1u - (b >> 3) : (b >> 3);
                        const uint32_t v = xcd_map(b, 8u * per, rev, s);
                        if (v != x * per + q || v != xcd_map(b, 8u * per, rev, 0u)) {
                            fail_msg("not contiguous eighths", 8u * per, rev, s, b, v);
                            break;
                        }
                    }
                }
        return done();
    }
    if (!std::strcmp(cmd, "clamp")) {
        for (int i = 2; i < argc; ++i) std::printf("%u\n", xcd_shift_clamp((int)std::strtol(argv[i], nullptr, 10)));
        return 0;
    }
    if (!std::strcmp(cmd, "map") && argc == 5) {
        const uint32_t grid = (uint32_t)std::strtoul(argv[2], nullptr, 10), rev = (uint32_t)std::atoi(argv[3]), shift = (uint32_t)std::atoi(argv[4]);
        for (uint32_t b = 0; b < grid; ++b) std::printf("%u\n", xcd_map(b, grid, rev, shift));
        return 0;
    }
    return 2;
}
