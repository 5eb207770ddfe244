// sphx_render.inc — the reference app's particle drawing on the device (sphx_render, include/sphx.h): every particle a disc, fluid over
// boundary over background, later fluid instances over earlier ones (main.rs:239-275), into an RGBA8 image and / or an owner image.
// Included at the end of sphx_kernels.hip (one translation unit: the launch layer of sphx_launch.inc is visible).  Compiled with
// -ffp-contract=off like the rest: the fp32 expressions are the contract of sphx.h, restated bit for bit by tests/render_reference.py.
//
// Shape: a scatter.  (1) clear one 32-bit word per pixel; (2) a sweep over the boundary and one over the fluid particles: cull, pixel
// rectangle (sphx_render_rect.hpp — the only float-to-index conversion), the contract's d2 <= r2 at exactly those pixel centres, and an
// atomic max of the encoded owner (0 none < 1 boundary < 2 + j) into each covered pixel; (3) a pass over the pixels decodes the word,
// gathers the owner's velocity and stores the packed colour and / or the owner.  The result is a pure function of the arrays and the
// view (max is order-independent), so it is the same bits whatever order the hardware takes.
#include "sphx_render_rect.hpp"
#include "sphx_render_window.hpp"

namespace sphx {

constexpr uint32_t RENDER_MAX_BLOCKS = 1u << 22;  // workgroups per launch (2^30 work-items, as SAMPLE_MAX_BLOCKS)

__global__ __launch_bounds__(256) void k_render_clear(uint32_t* __restrict__ code, uint32_t npix, uint32_t base) {
    const uint32_t p = base + blockIdx.x * 256u + threadIdx.x;
    if (p < npix) code[p] = 0u;
}

// Work-item t of the launch takes particle n - 1 - (base + t): the sweep runs from the highest index down, so that where several
// particles share a pixel the winner tends to arrive first and the others see it in the plain load in front of the atomic and skip
// theirs (a stale read only costs a redundant atomic: the word never decreases).  FLUID: the code is 2 + j, else 1 for every boundary
// particle.
//   Zoomed out, the lanes of a wavefront — Morton-consecutive particles — hit a handful of pixels between them, all at once, and the
// plain load sees nothing yet: left alone every lane fires its atomic and they serialise per address (1 343 us for the 16 M scene in
// 1920 x 1080, 87 particles per fluid pixel; DESIGN.md 4d).  So a wavefront whose rectangles are all small (<= RENDER_COMBINE x
// RENDER_COMBINE pixels) walks them in lockstep and combines first: of the lanes that cover the same pixel only the lowest — the
// highest index, the sweep descends — goes to memory.  A wavefront with a larger rectangle (zoomed in: a disc of tens of pixels, the
// lanes on different pixels) takes the plain per-lane loop.  Which path runs changes no bit: the word ends as the maximum either way.
constexpr uint32_t RENDER_COMBINE = 3;  // (3 x 3: what a disc of up to one pixel radius can touch)

__device__ __forceinline__ void render_put(uint32_t* word, uint32_t mine) {
    if (__atomic_load_n(word, __ATOMIC_RELAXED) < mine) atomicMax(word, mine);
}

// A tile's layer (sphx_tile_render_layer): what the scatter needs beyond the camera.  The tile draws what it OWNS — a fluid particle
// with bit 31 of its id, a boundary particle whose cell lies in the tile's rectangle — and keeps one word per pixel of its WINDOW only
// (sphx_render_window.hpp: every pixel an owned particle can cover lies in it), `ww` words per row, the window's first pixel at word 0.
struct RenderTile {
    const uint32_t* pid;              // particle_id[] of the fluid particles (not read by the boundary sweep)
    float gmin_x, gmin_y, cell_inv;   // the grid's cell function (cell_of)
    TileRect rect;                    // the tile's cells
    uint32_t wx0, wx1, wy0, wy1;      // the window: pixel columns [wx0, wx1), rows [wy0, wy1), inside the image, not empty
};
// (the single context's instantiations take an empty struct in its place, which occupies no kernel-argument space: their code is the code
// from before, profiles/render_multi/isa.txt)
template <bool TILE>
struct RenderTileArg {};
template <>
struct RenderTileArg<true> : RenderTile {};

template <bool FLUID, bool TILE = false>
__global__ __launch_bounds__(256) void k_render_scatter(const float2* __restrict__ pos, uint32_t n, RenderCam v, uint32_t* __restrict__ code,
                                                        uint32_t base, RenderTileArg<TILE> T) {
    const uint32_t t = base + blockIdx.x * 256u + threadIdx.x;
    const bool live = t < n;
    const uint32_t j = live ? n - 1u - t : 0u;
    RenderRect rc{0, 0, 0, 0};  // empty for everything off the image, for non-finite positions and for the lanes past the end
    float2 p = make_float2(0.0f, 0.0f);
    if (live) {
        p = pos[j];
        if constexpr (!TILE) {
            rc = render_pixel_rect(v, p.x, p.y);
        } else {
            bool drawn;
            if constexpr (FLUID) {
                drawn = T.pid[j] >> 31;  // a ghost: its owner draws it
            } else {
                const uint32_t cx = sat_u16((p.x - T.gmin_x) * T.cell_inv), cy = sat_u16((p.y - T.gmin_y) * T.cell_inv);  // cell_of()
                drawn = rect_has(T.rect, cx, cy, 0u);
            }
            if (drawn) rc = render_pixel_rect(v, p.x, p.y);
        }
        if constexpr (TILE) {  // ... intersected with the window: no word outside it exists
            rc.x0 = rc.x0 > T.wx0 ? rc.x0 : T.wx0, rc.x1 = rc.x1 < T.wx1 ? rc.x1 : T.wx1;
            rc.y0 = rc.y0 > T.wy0 ? rc.y0 : T.wy0, rc.y1 = rc.y1 < T.wy1 ? rc.y1 : T.wy1;
            if (rc.x0 >= rc.x1 || rc.y0 >= rc.y1) rc = RenderRect{T.wx0, T.wx0, T.wy0, T.wy0};  // (empty, and no index below the origin)
        }
    }
    if constexpr (TILE)
        if (!live) rc = RenderRect{T.wx0, T.wx0, T.wy0, T.wy0};
    const uint32_t mine = FLUID ? 2u + j : 1u;
    const uint32_t w = rc.x1 - rc.x0, h = rc.y1 - rc.y0;
    if (__any(w > RENDER_COMBINE || h > RENDER_COMBINE)) {
        for (uint32_t iy = rc.y0; iy < rc.y1; ++iy) {
            const float qy = render_qy(v, iy);
            uint32_t* row;  // (row + ix is the word of pixel (ix, iy): of the whole image, or of the tile's window)
            if constexpr (TILE)
                row = code + (size_t)(iy - T.wy0) * (T.wx1 - T.wx0) - T.wx0;
            else
                row = code + (size_t)iy * v.width;
            for (uint32_t ix = rc.x0; ix < rc.x1; ++ix)
                if (render_covers(v, p.x, p.y, render_qx(v, ix), qy)) render_put(row + ix, mine);
        }
        return;
    }
    // every lane looks at all its pixels first, the loads back to back (one round trip per wavefront, not one per pixel): a lane that
    // is beaten already drops out, and a wavefront that arrives late at its pixels sends nothing
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t seen[RENDER_COMBINE * RENDER_COMBINE];
#pragma unroll
    for (uint32_t dy = 0; dy < RENDER_COMBINE; ++dy) {
        const float qy = render_qy(v, rc.y0 + dy);
#pragma unroll
        for (uint32_t dx = 0; dx < RENDER_COMBINE; ++dx) {
            const bool cov = dy < h && dx < w && render_covers(v, p.x, p.y, render_qx(v, rc.x0 + dx), qy);
            // (only dereferenced when covered: a pixel inside the rectangle)
            uint32_t at;  // the pixel's word: of the whole image, or of the tile's window
            if constexpr (TILE)
                at = (rc.y0 + dy - T.wy0) * (T.wx1 - T.wx0) + (rc.x0 - T.wx0) + dx;
            else
                at = (rc.y0 + dy) * v.width + rc.x0 + dx;
            seen[dy * RENDER_COMBINE + dx] = cov ? __atomic_load_n(code + at, __ATOMIC_RELAXED) : 0xFFFFFFFFu;
        }
    }
#pragma unroll
    for (uint32_t dy = 0; dy < RENDER_COMBINE; ++dy) {
#pragma unroll
        for (uint32_t dx = 0; dx < RENDER_COMBINE; ++dx) {
            const bool need = seen[dy * RENDER_COMBINE + dx] < mine;  // (not covered: 0xFFFFFFFF, never below a code)
            uint32_t at;
            if constexpr (TILE)
                at = (rc.y0 + dy - T.wy0) * (T.wx1 - T.wx0) + (rc.x0 - T.wx0) + dx;
            else
                at = (rc.y0 + dy) * v.width + rc.x0 + dx;
            const uint32_t key = need ? at : 0xFFFFFFFFu;  // (< 2^28 for a pixel of the image)
            unsigned long long todo = __ballot(need);
            while (todo) {
                const uint32_t leader = (uint32_t)__ffsll(todo) - 1u;  // the lowest lane left = the highest index among its pixel's lanes
                const uint32_t k0 = (uint32_t)__shfl((int)key, (int)leader);
                if (lane == leader) atomicMax(code + k0, mine);  // (no value returned: nothing waits for it)
                todo &= ~__ballot(key == k0);
            }
        }
    }
}

// heatmap_color (main.rs:74-80) channel k of t, as a byte: clamp(t * 3 - k, 0, 1) with a NaN becoming 0
__device__ __forceinline__ uint32_t render_channel(float t, float k) {
    const float c = t * 3.0f - k;
    const float cc = c > 0.0f ? (c < 1.0f ? c : 1.0f) : 0.0f;
    return (uint32_t)(uint8_t)(cc * 255.0f + 0.5f);
}

__global__ __launch_bounds__(256) void k_render_resolve(const uint32_t* __restrict__ code, const float2* __restrict__ vel, uint32_t npix,
                                                        float speed_scale, uint32_t bg, uint32_t bd, uint32_t* __restrict__ rgba,
                                                        uint32_t* __restrict__ owner, uint32_t base) {
    const uint32_t p = base + blockIdx.x * 256u + threadIdx.x;
    if (p >= npix) return;
    const uint32_t c = code[p];
    if (owner) owner[p] = c >= 2u ? c - 2u : (c ? (uint32_t)SPHX_RENDER_BOUNDARY : (uint32_t)SPHX_RENDER_NONE);
    if (!rgba) return;
    uint32_t px = c ? bd : bg;
    if (c >= 2u) {
        const float2 w = vel[c - 2u];
        const float s = sqrtf(w.x * w.x + w.y * w.y);
        const float t = s * speed_scale;
        px = render_channel(t, 0.0f) | render_channel(t, 1.0f) << 8 | render_channel(t, 2.0f) << 16 | 0xFF000000u;
    }
    rgba[p] = px;  // bytes r, g, b, a in memory order
}

// The last pass of a tile's layer: the word of a pixel becomes (key, owner, rgba) — for a fluid owner j the Morton code of its cell (the
// grid's own fp32 cell function, morton.rs' encode), its id without the owner bit, and the colour exactly as k_render_resolve computes
// it.  FULL: one work-item per pixel of the VIEW, the outputs are full-size images and a pixel outside the window shows nothing;
// otherwise one per pixel of the window, the outputs are compact (the window's rows one after the other: what sphx_multi_render copies
// back).  Any output may be null.
template <bool FULL>
__global__ __launch_bounds__(256) void k_render_resolve_layer(const uint32_t* __restrict__ code, const float2* __restrict__ pos, const float2* __restrict__ vel,
                                                              const uint32_t* __restrict__ pid, uint32_t npix, uint32_t width, RenderTile T, float speed_scale,
                                                              uint32_t bg, uint32_t bd, uint32_t* __restrict__ key, uint32_t* __restrict__ owner,
                                                              uint32_t* __restrict__ rgba, uint32_t base) {
    const uint32_t p = base + blockIdx.x * 256u + threadIdx.x;
    if (p >= npix) return;
    uint32_t c = 0u;
    if constexpr (FULL) {
        const uint32_t iy = p / width, ix = p - iy * width;
        if (ix >= T.wx0 && ix < T.wx1 && iy >= T.wy0 && iy < T.wy1) c = code[(iy - T.wy0) * (T.wx1 - T.wx0) + (ix - T.wx0)];
    } else {
        c = code[p];
    }
    uint32_t k = 0u, o = c ? (uint32_t)SPHX_RENDER_BOUNDARY : (uint32_t)SPHX_RENDER_NONE, px = c ? bd : bg;
    if (c >= 2u) {
        const uint32_t j = c - 2u;
        const float2 x = pos[j];
        k = morton2(sat_u16((x.x - T.gmin_x) * T.cell_inv), sat_u16((x.y - T.gmin_y) * T.cell_inv));  // cell_of()
        o = pid[j] & 0x7FFFFFFFu;
        if (rgba) {
            const float2 w = vel[j];
            const float s = sqrtf(w.x * w.x + w.y * w.y);
            const float t = s * speed_scale;
            px = render_channel(t, 0.0f) | render_channel(t, 1.0f) << 8 | render_channel(t, 2.0f) << 16 | 0xFF000000u;
        }
    }
    if (key) key[p] = k;
    if (owner) owner[p] = o;
    if (rgba) rgba[p] = px;
}

}  // namespace sphx

// ---- launch layer and C ABI ----------------------------------------------------------------------------------------------------------
namespace {

inline uint32_t pack_rgba(const uint8_t* b) { return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24; }

// launches over `count` work-items in pieces of at most RENDER_MAX_BLOCKS workgroups
template <class F>
void render_pieces(sphx_ctx* c, const char* name, double bytes, uint64_t count, F&& f) {
    const uint64_t blocks = (count + 255u) / 256u;
    for (uint64_t b0 = 0; b0 < blocks; b0 += RENDER_MAX_BLOCKS) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(blocks - b0, RENDER_MAX_BLOCKS);
        launch(c, name, bytes * (double)nb / (double)blocks, [&] { f(nb, (uint32_t)(b0 * 256u)); });
    }
}

// the three passes on the context's stream; code: [npix] words of scratch, rgba / owner: device pointers or null
void enqueue_render(sphx_ctx* c, const RenderCam& v, const sphx_render_view& view, uint32_t* code, uint32_t* rgba, uint32_t* owner) {
    const uint32_t npix = v.width * v.height;
    const uint32_t rev = c->K.rev;  // (a render must not change the sweep direction of the step's next kernels: launch() toggles it)
    hipStream_t st = c->stream;
    render_pieces(c, "render_clear", 4.0 * npix, npix,
                  [&](uint32_t nb, uint32_t base) { hipLaunchKernelGGL(k_render_clear, dim3(nb), dim3(256), 0, st, code, npix, base); });
    if (c->B)
        render_pieces(c, "render_scatter", 8.0 * c->B, c->B, [&](uint32_t nb, uint32_t base) {
            hipLaunchKernelGGL((k_render_scatter<false, false>), dim3(nb), dim3(256), 0, st, (const float2*)c->bpos, c->B, v, code, base, RenderTileArg<false>{});
        });
    if (c->N)
        render_pieces(c, "render_scatter", 8.0 * c->N, c->N, [&](uint32_t nb, uint32_t base) {
            hipLaunchKernelGGL((k_render_scatter<true, false>), dim3(nb), dim3(256), 0, st, (const float2*)c->posA, c->N, v, code, base, RenderTileArg<false>{});
        });
    render_pieces(c, "render_resolve", (4.0 + (rgba ? 4.0 : 0.0) + (owner ? 4.0 : 0.0)) * npix, npix, [&](uint32_t nb, uint32_t base) {
        hipLaunchKernelGGL(k_render_resolve, dim3(nb), dim3(256), 0, st, (const uint32_t*)code, (const float2*)c->vel, npix, view.speed_scale,
                           pack_rgba(view.background), pack_rgba(view.boundary), rgba, owner, base);
    });
    c->K.rev = rev;
}

// the same passes for a tile's layer, over the window w (not empty unless `full`): clear and scatter touch the window's words only; the
// outputs are full-size images (full) or hold the window alone
void enqueue_render_layer(sphx_ctx* c, const RenderCam& v, const sphx_render_view& view, const RenderWindow& w, bool full, uint32_t* code, uint32_t* key,
                          uint32_t* owner, uint32_t* rgba) {
    const uint32_t npw = (uint32_t)w.pixels(), npix = full ? v.width * v.height : npw;
    const uint32_t rev = c->K.rev;
    hipStream_t st = c->stream;
    RenderTileArg<true> T;
    T.pid = c->pid;
    T.gmin_x = c->K.gmin_x, T.gmin_y = c->K.gmin_y, T.cell_inv = c->K.cell_inv;
    T.rect = c->K.tile;
    T.wx0 = w.x0, T.wx1 = w.x1, T.wy0 = w.y0, T.wy1 = w.y1;
    if (npw) {
        render_pieces(c, "render_clear", 4.0 * npw, npw,
                      [&](uint32_t nb, uint32_t base) { hipLaunchKernelGGL(k_render_clear, dim3(nb), dim3(256), 0, st, code, npw, base); });
        if (c->B)
            render_pieces(c, "render_scatter_tile", 8.0 * c->B, c->B, [&](uint32_t nb, uint32_t base) {
                hipLaunchKernelGGL((k_render_scatter<false, true>), dim3(nb), dim3(256), 0, st, (const float2*)c->bpos, c->B, v, code, base, T);
            });
        if (c->N)
            render_pieces(c, "render_scatter_tile", 12.0 * c->N, c->N, [&](uint32_t nb, uint32_t base) {
                hipLaunchKernelGGL((k_render_scatter<true, true>), dim3(nb), dim3(256), 0, st, (const float2*)c->posA, c->N, v, code, base, T);
            });
    }
    if (npix)
        render_pieces(c, "render_resolve_layer", (4.0 + (key ? 4.0 : 0.0) + (owner ? 4.0 : 0.0) + (rgba ? 4.0 : 0.0)) * npix, npix, [&](uint32_t nb, uint32_t base) {
            if (full)
                hipLaunchKernelGGL(k_render_resolve_layer<true>, dim3(nb), dim3(256), 0, st, (const uint32_t*)code, (const float2*)c->posA, (const float2*)c->vel,
                                   (const uint32_t*)c->pid, npix, v.width, (RenderTile)T, view.speed_scale, pack_rgba(view.background), pack_rgba(view.boundary), key,
                                   owner, rgba, base);
            else
                hipLaunchKernelGGL(k_render_resolve_layer<false>, dim3(nb), dim3(256), 0, st, (const uint32_t*)code, (const float2*)c->posA, (const float2*)c->vel,
                                   (const uint32_t*)c->pid, npix, v.width, (RenderTile)T, view.speed_scale, pack_rgba(view.background), pack_rgba(view.boundary), key,
                                   owner, rgba, base);
        });
    c->K.rev = rev;
}

// the context's render scratch, grown to `need` words (a queued render may still use the old one)
int render_scratch(sphx_ctx* c, size_t need) {
    if (need <= c->render_cap) return SPHX_OK;
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    int rc;
    if ((rc = dev_alloc(c, &c->render_buf, need))) {
        c->render_cap = 0;
        return rc;
    }
    c->render_cap = need;
    return SPHX_OK;
}

// the rules of a tile layer call up to the point where work begins: SPHX_OK go on, RENDER_NOOP a successful no-op (no pixels), else the
// error code of the refusal
constexpr int RENDER_NOOP = -1;  // (no status code is negative)
int render_tile_ready(sphx_ctx* c, const char* fn, const sphx_render_view* view, uint32_t flags, uint32_t allowed) {
    if (!view) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "view is NULL");
    if (flags & ~allowed) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "unknown flags bits");
    if (!c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not a tile context (sphx_render serves a plain one)");
    if (const char* bad = render_view_error(view, c->P.smoothing_length)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, bad);
    if (c->N > 0xFFFFFFFDu) return c->fail(SPHX_ERR_CAPACITY, fn, "more than 2^32 - 3 particles (two owner codes are taken)");
    if ((uint64_t)view->width * view->height == 0) return RENDER_NOOP;
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, fn, "between step_begin and step_finish (finish the step first)");
    // between the packing pass and the re-grid the local count is an upper bound and an advection may be pending (as sphx_tile_fluid_stats)
    if (c->N && (!c->lists_current || c->tile_pending_dt > 0.0f))
        return c->fail(SPHX_ERR_NOT_READY, fn, "the tile is between a halo exchange and its re-grid (sphx_sub_regrid first)");
    return SPHX_OK;
}

}  // namespace

extern "C" {

int sphx_render(sphx_ctx* c, const sphx_render_view* view, uint32_t flags, const sphx_render_out* out) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!view) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_render: view is NULL");
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_render: out is NULL");
    if (!out->rgba && !out->owner) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_render: out requests no output (rgba and owner are NULL)");
    if (flags & ~(uint32_t)SPHX_RENDER_DEVICE_POINTERS) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_render: unknown flags bits");
    if (c->tile_mode)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_render: not available on a tile context (its arrays hold ghosts and miss the particles other tiles own)");
    if (const char* bad = render_view_error(view, c->P.smoothing_length)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_render", bad);
    const uint64_t npix = (uint64_t)view->width * view->height;
    if (c->N > 0xFFFFFFFDu) return c->fail(SPHX_ERR_CAPACITY, "sphx_render: more than 2^32 - 3 particles (two owner codes are taken)");
    if (npix == 0) return SPHX_OK;
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, "sphx_render: between step_begin and step_finish (finish the step first)");
    SPHX_HIP(c, hipSetDevice(c->device));
    flush_pending_advect(c);

    const RenderCam v = render_make_cam(*view, c->P.particle_radius);

    // scratch: the owner codes, and on the host-pointer path the device copies of the outputs behind them
    const bool dev = flags & SPHX_RENDER_DEVICE_POINTERS;
    int rc;
    if ((rc = render_scratch(c, (size_t)npix * (1u + (!dev && out->rgba ? 1u : 0u) + (!dev && out->owner ? 1u : 0u))))) return rc;
    uint32_t* const code = c->render_buf;
    if (dev) {
        enqueue_render(c, v, *view, code, (uint32_t*)out->rgba, out->owner);
        return SPHX_OK;
    }
    uint32_t* p = code + npix;
    uint32_t* const d_rgba = out->rgba ? p : nullptr;
    if (out->rgba) p += npix;
    uint32_t* const d_owner = out->owner ? p : nullptr;
    enqueue_render(c, v, *view, code, d_rgba, d_owner);
    if (d_rgba) SPHX_HIP(c, hipMemcpyAsync(out->rgba, d_rgba, (size_t)npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (d_owner) SPHX_HIP(c, hipMemcpyAsync(out->owner, d_owner, (size_t)npix * 4, hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    return SPHX_OK;
}

int sphx_tile_render_layer(sphx_ctx* c, const sphx_render_view* view, uint32_t flags, const sphx_render_layer* out) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_render_layer";
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out is NULL");
    if (!out->key && !out->owner && !out->rgba) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out requests no output (key, owner and rgba are NULL)");
    int rc;
    if ((rc = render_tile_ready(c, fn, view, flags, (uint32_t)SPHX_RENDER_DEVICE_POINTERS))) return rc == RENDER_NOOP ? SPHX_OK : rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    const RenderCam v = render_make_cam(*view, c->P.particle_radius);
    const RenderWindow w = render_tile_window(v, c->K.tile.x0, c->K.tile.x1, c->K.tile.y0, c->K.tile.y1, c->K.gmin_x, c->K.gmin_y, c->K.cell_inv);
    const size_t npix = (size_t)view->width * view->height, npw = (size_t)w.pixels();
    const bool dev = flags & SPHX_RENDER_DEVICE_POINTERS;
    const uint32_t n_out = (out->key ? 1u : 0u) + (out->owner ? 1u : 0u) + (out->rgba ? 1u : 0u);
    if ((rc = render_scratch(c, npw + (dev ? 0u : npix * n_out)))) return rc;
    uint32_t* const code = c->render_buf;
    if (dev) {
        enqueue_render_layer(c, v, *view, w, true, code, out->key, out->owner, (uint32_t*)out->rgba);
        return SPHX_OK;
    }
    uint32_t* p = code + npw;
    uint32_t* const d_key = out->key ? p : nullptr;
    if (out->key) p += npix;
    uint32_t* const d_owner = out->owner ? p : nullptr;
    if (out->owner) p += npix;
    uint32_t* const d_rgba = out->rgba ? p : nullptr;
    enqueue_render_layer(c, v, *view, w, true, code, d_key, d_owner, d_rgba);
    if (d_key) SPHX_HIP(c, hipMemcpyAsync(out->key, d_key, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (d_owner) SPHX_HIP(c, hipMemcpyAsync(out->owner, d_owner, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (d_rgba) SPHX_HIP(c, hipMemcpyAsync(out->rgba, d_rgba, npix * 4, hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    return SPHX_OK;
}

int sphx_tile_render_window(sphx_ctx* c, const sphx_render_view* view, uint32_t want_rgba, uint32_t* out_window, sphx_render_layer* out_dev) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_render_window";
    if (!out_window || !out_dev) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out_window or out_dev is NULL");
    out_window[0] = out_window[1] = out_window[2] = out_window[3] = 0u;
    out_dev->key = out_dev->owner = nullptr;
    out_dev->rgba = nullptr;
    int rc;
    if ((rc = render_tile_ready(c, fn, view, 0u, 0u))) return rc == RENDER_NOOP ? SPHX_OK : rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    const RenderCam v = render_make_cam(*view, c->P.particle_radius);
    const RenderWindow w = render_tile_window(v, c->K.tile.x0, c->K.tile.x1, c->K.tile.y0, c->K.tile.y1, c->K.gmin_x, c->K.gmin_y, c->K.cell_inv);
    const size_t npw = (size_t)w.pixels();
    if (!npw) return SPHX_OK;  // nothing this tile owns can reach the image
    if ((rc = render_scratch(c, npw * (want_rgba ? 4u : 3u)))) return rc;
    uint32_t* const code = c->render_buf;
    out_dev->key = code + npw;
    out_dev->owner = code + 2 * npw;
    out_dev->rgba = want_rgba ? (uint8_t*)(code + 3 * npw) : nullptr;
    enqueue_render_layer(c, v, *view, w, false, code, out_dev->key, out_dev->owner, (uint32_t*)out_dev->rgba);
    out_window[0] = w.x0, out_window[1] = w.x1, out_window[2] = w.y0, out_window[3] = w.y1;
    return SPHX_OK;
}

}  // extern "C"
