// sphx_render_rect.hpp — the one place where sphx_render (include/sphx.h) turns a float into a pixel index: the conservative pixel
// rectangle of a disc.  Shared by the scatter kernel (sphx_render.inc) and a host driver (tests/render_rect_driver.cpp) that feeds it
// hostile values before the kernel ever runs: a mistake here is a store outside the image.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPHX_RECT_HD __host__ __device__
#else
#define SPHX_RECT_HD
#endif

namespace sphx {

// what the scatter needs of a sphx_render_view (derived once, on the host)
struct RenderCam {
    float cx, cy;   // view.center
    float ppu;      // view.pixel_per_world_unit
    float inv;      // 1.0f / ppu
    float r, r2;    // disc radius in world units (max(radius, min_pixel_radius * inv)) and its square
    uint32_t width, height;
};

// pixel columns [x0, x1) and rows [y0, y1), 0 <= x0 <= x1 <= width, 0 <= y0 <= y1 <= height; empty = all zero
struct RenderRect {
    uint32_t x0, x1, y0, y1;
};

// The pixel centre of (ix, iy) in world coordinates: the contract's expression, fp32 and unfused.
SPHX_RECT_HD inline float render_qx(const RenderCam& v, uint32_t ix) { return v.cx + (((float)ix + 0.5f) - 0.5f * (float)v.width) * v.inv; }
SPHX_RECT_HD inline float render_qy(const RenderCam& v, uint32_t iy) { return v.cy - (((float)iy + 0.5f) - 0.5f * (float)v.height) * v.inv; }
// ... and the coverage test at it.  A non-finite position gives a NaN or an infinite d2: false.
SPHX_RECT_HD inline bool render_covers(const RenderCam& v, float px, float py, float qx, float qy) {
    const float dx = px - qx, dy = py - qy;
    const float d2 = dx * dx + dy * dy;
    return d2 <= v.r2;
}

// One axis: the indices i in [0, n) whose centre i + 0.5 can lie within the disc's half width of the particle's screen coordinate
// s = off * ppu + n / 2 (off = particle - centre along the axis, sign already that of the screen axis).
//   half = the radius in pixels, plus everything fp32 can have moved: the contract evaluates the test at q = c + (...) * inv, which is
//   rounded to an ulp of |c| + |p| + r world units (2^-24 relative each for inv, the product and the sum; 2^-23 of n in (float)i for
//   n >= 2^24), s here is rounded likewise, and d2 <= r2 carries ~2^-22 of r.  `err` bounds the sum of those in pixels with a factor
//   of at least 4 to spare; the 0.01 covers the rest for small numbers.
// Everything is clamped to [0, n] as a FLOAT before the conversion; a NaN anywhere fails the first comparison and gives the empty
// range.  Returns lo <= hi <= n.
SPHX_RECT_HD inline void render_axis_range(float off, float absp, float absc, const RenderCam& v, uint32_t n, uint32_t& lo, uint32_t& hi) {
    const float fn = (float)n;
    const float s = off * v.ppu + 0.5f * fn;
    const float err = ((absp + absc + v.r) * v.ppu + fn) * 4.76837158203125e-7f;  // 2^-21
    const float half = (v.r * v.ppu) * 1.00001f + err + 0.01f;
    const float a = (s - half) - 0.5f, b = (s + half) - 0.5f;  // i + 0.5 in [s - half, s + half]  <=>  i in [a, b]
    lo = hi = 0;
    if (!(b >= 0.0f && a <= fn)) return;  // off the image, or NaN (inf - inf)
    const float fa = a > 0.0f ? a : 0.0f, fb = b < fn ? b : fn;  // 0 <= fa, fb <= fn < 2^28: the conversions below are exact
    uint32_t i0 = (uint32_t)fa, i1 = (uint32_t)fb + 1u;           // floor(a) (one column more than ceil(a): no rounding case to argue), floor(b) + 1
    if (i1 > n) i1 = n;
    if (i0 > i1) i0 = i1;
    lo = i0;
    hi = i1;
}

SPHX_RECT_HD inline float render_abs(float x) { return x < 0.0f ? -x : x; }

SPHX_RECT_HD inline RenderRect render_pixel_rect(const RenderCam& v, float px, float py) {
    RenderRect rc{0, 0, 0, 0};
    uint32_t x0, x1, y0, y1;
    render_axis_range(px - v.cx, render_abs(px), render_abs(v.cx), v, v.width, x0, x1);
    if (x0 == x1) return rc;
    render_axis_range(v.cy - py, render_abs(py), render_abs(v.cy), v, v.height, y0, y1);  // screen y grows downwards (camera.rs:49)
    if (y0 == y1) return rc;
    rc.x0 = x0, rc.x1 = x1, rc.y0 = y0, rc.y1 = y1;
    return rc;
}

}  // namespace sphx
