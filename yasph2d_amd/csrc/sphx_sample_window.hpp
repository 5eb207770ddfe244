// sphx_sample_window.hpp — the WINDOW of a tile in a sampling lattice (sphx_multi_sample_grid, include/sphx.h): the index rectangle
// [ix0, ix1) x [iy0, iy1) of the lattice points whose cell lies in a tile's owned cell rectangle.  Plain C++ without a GPU call, compiled
// into the kernels' translation unit, into sphx_tiles.cpp and into tests/sample_window_driver.cpp, which compares it with the brute-force
// set before any kernel runs: a window that is too small loses points, one that is too large hands a point to two tiles.
//
// The cell of lattice index i along one axis is sat_u16((fl(o + fl(fl((float)i) * d)) - gmin) * cell_inv) — the device's expression
// (k_sample_grid, cell_of), every operation rounded to fp32 on its own.  With d > 0 and cell_inv > 0 each of those operations is
// monotone non-decreasing in its varying operand (rounding is monotone; an overflow to +inf stays +inf through the rest and saturates
// to cell 65535; no NaN can arise from a finite origin), so the cell is monotone in i and the indices of any cell interval are
// contiguous: two bisections per axis find them.  MUST be compiled with floating-point contraction off: a fused o + i * d is a
// different point.  The pragma below says so to clang; the project's flags (-ffp-contract=off) say it to every compiler, and the driver
// is built with the same flag.
#pragma once
#include <cmath>
#include <cstdint>

namespace sphx_sample_host {

// Rust `f32 as u16` as the device evaluates it (sat_u16, sphx_kernels.hip): saturating, NaN -> 0
inline uint32_t sat_u16(float v) {
    v = std::fmin(std::fmax(v, 0.0f), 65535.0f);
    return (uint32_t)v;
}

// cell coordinate of the point with coordinate q
inline uint32_t cell_coord(float q, float gmin, float cell_inv) {
#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif
    return sat_u16((q - gmin) * cell_inv);
}

// coordinate of lattice index i along one axis: o + (float)i * d, unfused
inline float lattice_coord(float o, float d, uint32_t i) {
#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif
    const float t = (float)i * d;
    return o + t;
}

inline uint32_t lattice_cell(float o, float d, uint32_t i, float gmin, float cell_inv) { return cell_coord(lattice_coord(o, d, i), gmin, cell_inv); }

// the first index i of [0, n] whose cell is >= c (n: none is); the cell is monotone in i
inline uint32_t first_cell_at_least(float o, float d, uint32_t n, float gmin, float cell_inv, uint32_t c) {
    uint32_t lo = 0, hi = n;  // every index below lo has a cell < c, every index from hi on a cell >= c
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (lattice_cell(o, d, mid, gmin, cell_inv) >= c)
            hi = mid;
        else
            lo = mid + 1u;
    }
    return lo;
}

// indices [i0, i1) of [0, n) whose cell lies in [c0, c1); c1 may be 65536 (every cell is <= 65535).  i0 <= i1 <= n.
inline void axis_window(float o, float d, uint32_t n, float gmin, float cell_inv, uint32_t c0, uint32_t c1, uint32_t& i0, uint32_t& i1) {
    if (c0 >= c1) {
        i0 = i1 = 0;
        return;
    }
    i0 = first_cell_at_least(o, d, n, gmin, cell_inv, c0);
    i1 = c1 > 65535u ? n : first_cell_at_least(o, d, n, gmin, cell_inv, c1);
    if (i1 < i0) i1 = i0;  // (cannot happen for a monotone cell function)
}

struct Window {
    uint32_t ix0, ix1, iy0, iy1;
    uint32_t w() const { return ix1 - ix0; }
    uint32_t h() const { return iy1 - iy0; }
    uint64_t points() const { return (uint64_t)(ix1 - ix0) * (iy1 - iy0); }
};

// the window of the cell rectangle [cx0, cx1) x [cy0, cy1) in the lattice (x0, y0, dx, dy, nx, ny); all zero if it is empty
inline Window lattice_window(float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, float gmin_x, float gmin_y, float cell_inv, uint32_t cx0,
                             uint32_t cx1, uint32_t cy0, uint32_t cy1) {
    Window w;
    axis_window(x0, dx, nx, gmin_x, cell_inv, cx0, cx1, w.ix0, w.ix1);
    axis_window(y0, dy, ny, gmin_y, cell_inv, cy0, cy1, w.iy0, w.iy1);
    if (w.ix0 == w.ix1 || w.iy0 == w.iy1) w = Window{0, 0, 0, 0};
    return w;
}

// ---- the fold of the ranks' parts (sphx_sample_merge, include/sphx.h) -------------------------------------------------------------------
struct Part {
    const uint32_t* density;   // bit patterns: the values cross the fold as integers
    const uint32_t* fraction;
    const uint32_t* velocity;
    const uint32_t* count;
    const int32_t* tile;
};
struct Acc {
    uint32_t *density, *fraction, *velocity, *count;
    int32_t* tile;
};
// Entry k of the answer: the part with tile[k] >= 0, the lowest tile if several have one (equal tiles: the earlier part); none: zeros
// and tile -1.  Entry k of the answer depends on entry k of the parts alone and is written after they are read: out may alias a part.
inline void merge(uint32_t m, const Part* parts, uint32_t n_parts, const Acc& out) {
    for (uint32_t k = 0; k < m; ++k) {
        const Part* best = nullptr;
        for (uint32_t p = 0; p < n_parts; ++p)
            if (parts[p].tile[k] >= 0 && (!best || parts[p].tile[k] < best->tile[k])) best = &parts[p];
        const uint32_t d = best && out.density ? best->density[k] : 0u, f = best && out.fraction ? best->fraction[k] : 0u;
        const uint32_t vx = best && out.velocity ? best->velocity[2 * (size_t)k] : 0u, vy = best && out.velocity ? best->velocity[2 * (size_t)k + 1] : 0u;
        const uint32_t c = best && out.count ? best->count[k] : 0u;
        const int32_t t = best ? best->tile[k] : -1;
        if (out.density) out.density[k] = d;
        if (out.fraction) out.fraction[k] = f;
        if (out.velocity) out.velocity[2 * (size_t)k] = vx, out.velocity[2 * (size_t)k + 1] = vy;
        if (out.count) out.count[k] = c;
        if (out.tile) out.tile[k] = t;
    }
}

}  // namespace sphx_sample_host
