// sphx_gauge_window.hpp — the INTERVAL of a tile on a gauge (sphx_multi_gauge_levels, include/sphx.h): the sample indices [lo, lo + count)
// of a ray whose cell lies in a tile's owned cell rectangle.  Plain C++ without a GPU call, compiled into the kernels' translation unit,
// into sphx_tiles.cpp and into tests/gauge_merge_driver.cpp, which compares it with the brute-force owned set before any kernel runs.
//
// FACT 1: the owned samples of one tile on one gauge are ONE contiguous index interval.
//   Sample k of a gauge is (x0 + fl((float)k * dx), y0 + fl((float)k * dy)), unfused, and the cell of a coordinate q is
//   sat_u16(fl(fl(q - gmin) * cell_inv)) — the device's cell_of().  For a finite step d and cell_inv > 0 every one of these operations is
//   monotone in its varying operand (k < 2^24 converts exactly; rounding is monotone): the cell is non-decreasing in k for d > 0,
//   non-increasing for d < 0 and constant for d == +-0.  An overflow of k * d to +-inf stays +-inf through the sum with a finite origin
//   and saturates to cell 65535 or 0; no NaN can arise (0 * d = 0 for finite d, and no inf - inf).  This is the argument of
//   sphx_sample_window.hpp, read for either sign.  So the indices of a cell interval [c0, c1) along one axis are contiguous, a tile owns a
//   cell RECTANGLE, and its samples are the intersection of two contiguous intervals: four bisections per gauge and tile.
// FACT 2: the rectangles of a tiling are disjoint and cover the u16 cell domain, so the intervals of the tiles on one gauge are disjoint
//   and cover [0, n): every sample is owned exactly once.  If the tile that owns sample `last` does not own last + 1, then last + 1 is
//   the FIRST owned sample of the tile that does — a partial that carries the value at its own first sample is enough for the fold
//   (sphx_gauge_merge.hpp).
// MUST be compiled with floating-point contraction off (a fused o + k * d is a different point), like sphx_sample_window.hpp, whose
// cell_coord / lattice_coord these functions call.
#pragma once
#include <algorithm>
#include <cstdint>

#include "sphx_sample_window.hpp"

namespace sphx_gauge_host {

// the first index of [0, n] from which on the cell is >= c (step >= 0: the cell does not decrease) resp. < c (step < 0: it does not
// increase); n: none is
inline uint32_t first_past(float o, float d, uint32_t n, float gmin, float cell_inv, uint32_t c, bool falling) {
    uint32_t lo = 0, hi = n;  // every index below lo fails the test, every index from hi on passes it
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        const uint32_t cell = sphx_sample_host::lattice_cell(o, d, mid, gmin, cell_inv);
        if (falling ? cell < c : cell >= c)
            hi = mid;
        else
            lo = mid + 1u;
    }
    return lo;
}

// indices [i0, i1) of [0, n) whose cell lies in [c0, c1) along one axis, for a step of either sign or zero; c1 may be 65536
inline void axis_interval(float o, float d, uint32_t n, float gmin, float cell_inv, uint32_t c0, uint32_t c1, uint32_t& i0, uint32_t& i1) {
    if (c0 >= c1) {
        i0 = i1 = 0;
        return;
    }
    if (d < 0.0f) {  // non-increasing: the cells < c1 begin at i0, the cells < c0 at i1
        i0 = c1 > 65535u ? 0u : first_past(o, d, n, gmin, cell_inv, c1, true);
        i1 = c0 == 0u ? n : first_past(o, d, n, gmin, cell_inv, c0, true);
    } else {  // non-decreasing (constant for d == +-0)
        i0 = first_past(o, d, n, gmin, cell_inv, c0, false);
        i1 = c1 > 65535u ? n : first_past(o, d, n, gmin, cell_inv, c1, false);
    }
    if (i1 < i0) i1 = i0;  // (cannot happen for a monotone cell function)
}

struct Interval {
    uint32_t lo, count;  // samples [lo, lo + count); count == 0: none (lo is then 0)
};

// the samples of the ray (x0, y0, dx, dy, n) whose cell lies in [cx0, cx1) x [cy0, cy1)
inline Interval gauge_interval(float x0, float y0, float dx, float dy, uint32_t n, float gmin_x, float gmin_y, float cell_inv, uint32_t cx0, uint32_t cx1,
                               uint32_t cy0, uint32_t cy1) {
    uint32_t a0, a1, b0, b1;
    axis_interval(x0, dx, n, gmin_x, cell_inv, cx0, cx1, a0, a1);
    axis_interval(y0, dy, n, gmin_y, cell_inv, cy0, cy1, b0, b1);
    const uint32_t lo = std::max(a0, b0), hi = std::min(a1, b1);
    return lo < hi ? Interval{lo, hi - lo} : Interval{0u, 0u};
}

// brute force, for the tests: is sample k of the ray in the rectangle? (the device's test, rect_has(K.tile, cell_of(q)))
inline bool sample_owned(float x0, float y0, float dx, float dy, uint32_t k, float gmin_x, float gmin_y, float cell_inv, uint32_t cx0, uint32_t cx1,
                         uint32_t cy0, uint32_t cy1) {
    const uint32_t cx = sphx_sample_host::lattice_cell(x0, dx, k, gmin_x, cell_inv), cy = sphx_sample_host::lattice_cell(y0, dy, k, gmin_y, cell_inv);
    return cx >= cx0 && cx < cx1 && cy >= cy0 && cy < cy1;
}

}  // namespace sphx_gauge_host
