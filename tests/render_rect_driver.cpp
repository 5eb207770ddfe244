// Host driver of tests/test_render_host.py: the pixel rectangle of sphx_render's scatter (yasph2d_amd/csrc/sphx_render_rect.hpp),
// compiled as plain C++ so that hostile values reach it before the kernel ever runs on a GPU.
// Reads binary records from stdin until it ends: {u32 width, u32 height, f32 cx, f32 cy, f32 pixel_per_world_unit, f32 r, u32 n} followed
// by n particles {f32 x, f32 y}; writes {u32 x0, x1, y0, y1} per particle to stdout.  inv and r2 are derived as the library derives them.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sphx_render_rect.hpp"

int main() {
    struct Head {
        uint32_t width, height;
        float cx, cy, ppu, r;
        uint32_t n;
    } h;
    while (std::fread(&h, sizeof(h), 1, stdin) == 1) {
        std::vector<float> xy(2 * (size_t)h.n);
        if (h.n && std::fread(xy.data(), 8, h.n, stdin) != h.n) return 1;
        sphx::RenderCam v;
        v.cx = h.cx, v.cy = h.cy, v.ppu = h.ppu;
        v.inv = 1.0f / h.ppu;
        v.r = h.r, v.r2 = h.r * h.r;
        v.width = h.width, v.height = h.height;
        std::vector<sphx::RenderRect> out(h.n);
        for (uint32_t i = 0; i < h.n; ++i) out[i] = sphx::render_pixel_rect(v, xy[2 * i], xy[2 * i + 1]);
        if (h.n && std::fwrite(out.data(), sizeof(sphx::RenderRect), h.n, stdout) != h.n) return 1;
    }
    return 0;
}
