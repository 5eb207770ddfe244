// sphx_render_window.hpp — what sphx_render and the tile layers (sphx_tile_render_layer, sphx_multi_render: include/sphx.h) share on
// the host: the argument rules of a view, the camera derived from it, and the WINDOW of a tile — the pixel rectangle the particles of a
// cell rectangle can reach, the second place (after sphx_render_rect.hpp) where a float becomes a pixel index.  Plain C++ without a GPU
// call, compiled into the kernels' translation unit, into sphx_tiles.cpp and into tests/render_merge_driver.cpp, which feeds the window
// with hostile values before any kernel runs: a window that is too small loses pixels, one whose indices leave the image is a store
// outside the scratch array.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#include "../../include/sphx.h"
#include "sphx_render_rect.hpp"

namespace sphx {

// The argument rules of a view (sphx_render's, in its order).  Returns the message behind "<function>: ", or nullptr.
inline const char* render_view_error(const sphx_render_view* view, float smoothing_length) {
    if (!std::isfinite(view->pixel_per_world_unit) || !(view->pixel_per_world_unit > 0.0f)) return "view.pixel_per_world_unit must be finite and > 0";
    if (!std::isfinite(view->center[0]) || !std::isfinite(view->center[1])) return "view.center must be finite";
    if (!std::isfinite(view->radius) || view->radius < 0.0f || view->radius > smoothing_length) return "view.radius must be finite and in [0, smoothing_length]";
    if (!std::isfinite(view->min_pixel_radius) || view->min_pixel_radius < 0.0f || view->min_pixel_radius > 4.0f)
        return "view.min_pixel_radius must be finite and in [0, 4]";
    if (!std::isfinite(view->speed_scale)) return "view.speed_scale must be finite";
    if ((uint64_t)view->width * view->height >= (1ull << 28)) return "view.width * view.height must be < 2^28";
    return nullptr;
}

// the camera of a checked view (the contract's r = max(radius != 0 ? radius : particle_radius, min_pixel_radius * inv))
inline RenderCam render_make_cam(const sphx_render_view& view, float particle_radius) {
    RenderCam v;
    v.cx = view.center[0], v.cy = view.center[1];
    v.ppu = view.pixel_per_world_unit;
    v.inv = 1.0f / view.pixel_per_world_unit;
    const float r_world = view.radius > 0.0f ? view.radius : particle_radius, r_pixel = view.min_pixel_radius * v.inv;
    v.r = r_world > r_pixel ? r_world : r_pixel;
    v.r2 = v.r * v.r;
    v.width = view.width, v.height = view.height;
    return v;
}

// pixel columns [x0, x1) and rows [y0, y1) of the image, x0 <= x1 <= width, y0 <= y1 <= height; may be empty
struct RenderWindow {
    uint32_t x0, x1, y0, y1;
    uint32_t w() const { return x1 - x0; }
    uint32_t h() const { return y1 - y0; }
    uint64_t pixels() const { return (uint64_t)(x1 - x0) * (y1 - y0); }
};

// One axis: the pixel indices [i0, i1) of [0, n) that a disc of radius r around a particle whose coordinate lies in [lo, hi] (world
// units; -inf / +inf: unbounded) can cover.  c: the view's centre along the axis, flip: the screen axis runs against the world axis
// (rows).  In double: the screen coordinate s = (p - c) * ppu + n / 2 of an end, the radius in pixels, and a slack of two pixels plus
// 2^-20 of every magnitude that enters the contract's fp32 expressions (sphx_render_rect.hpp bounds their error by 2^-21 of the same
// sum).  Anything that is not a number leaves the whole axis: too large a window only costs time.  Returns i0 <= i1 <= n.
inline void render_window_axis(double lo, double hi, double c, double ppu, double r, uint32_t n, bool flip, uint32_t& i0, uint32_t& i1) {
    const double fn = (double)n;
    i0 = 0, i1 = n;
    const double a = flip ? c - hi : lo - c, b = flip ? c - lo : hi - c;  // the ends on the screen axis, in world units from the centre
    const double mag = (std::isfinite(lo) ? std::fabs(lo) : 0.0) + (std::isfinite(hi) ? std::fabs(hi) : 0.0) + std::fabs(c) + r;
    const double slack = r * ppu * 1.00001 + 2.0 + (mag * ppu + fn) * 9.5367431640625e-7;  // 2^-20
    const double fa = (a * ppu + 0.5 * fn - slack) - 0.5, fb = (b * ppu + 0.5 * fn + slack) - 0.5;  // pixel i is reachable only if fa <= i <= fb
    if (fa > 0.0) i0 = fa >= fn ? n : (uint32_t)fa;          // (0 < fa < fn <= 2^32: the conversion is defined; a NaN fails the test)
    if (fb < fn) i1 = fb < 0.0 ? 0u : (uint32_t)fb + 1u;     // floor(fb) + 1 <= n
    if (i1 > n) i1 = n;
    if (i0 > i1) i0 = i1;
}

// The window of the cell rectangle [cx0, cx1) x [cy0, cy1) of the grid (origin gmin, cell_inv = 1 / cell size as the grid's own fp32
// cell function uses it): a particle of cell k has its coordinate in [gmin + k * cell, gmin + (k + 1) * cell) up to the rounding of
// (p - gmin) * cell_inv — a cell index is below 2^16 and fp32 carries 24 bits, so one cell of margin on either side covers it many times
// over.  An edge at 0 or 65536 is unbounded: the saturated cells hold the particles from anywhere beyond the domain.
inline RenderWindow render_tile_window(const RenderCam& v, uint32_t cx0, uint32_t cx1, uint32_t cy0, uint32_t cy1, float gmin_x, float gmin_y, float cell_inv) {
    const double inf = std::numeric_limits<double>::infinity();
    const double cell = 1.0 / (double)cell_inv;
    const double lox = cx0 == 0u ? -inf : (double)gmin_x + ((double)cx0 - 1.0) * cell, hix = cx1 >= 65536u ? inf : (double)gmin_x + ((double)cx1 + 1.0) * cell;
    const double loy = cy0 == 0u ? -inf : (double)gmin_y + ((double)cy0 - 1.0) * cell, hiy = cy1 >= 65536u ? inf : (double)gmin_y + ((double)cy1 + 1.0) * cell;
    RenderWindow w;
    render_window_axis(lox, hix, (double)v.cx, (double)v.ppu, (double)v.r, v.width, false, w.x0, w.x1);
    render_window_axis(loy, hiy, (double)v.cy, (double)v.ppu, (double)v.r, v.height, true, w.y0, w.y1);
    if (cx0 >= cx1 || cy0 >= cy1 || w.x0 == w.x1 || w.y0 == w.y1) w = RenderWindow{0, 0, 0, 0};  // nothing owned, or nothing of it on the image
    return w;
}

}  // namespace sphx
