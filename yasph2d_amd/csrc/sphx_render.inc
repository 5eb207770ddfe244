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

template <bool FLUID>
__global__ __launch_bounds__(256) void k_render_scatter(const float2* __restrict__ pos, uint32_t n, RenderCam v, uint32_t* __restrict__ code,
                                                        uint32_t base) {
    const uint32_t t = base + blockIdx.x * 256u + threadIdx.x;
    const bool live = t < n;
    const uint32_t j = live ? n - 1u - t : 0u;
    RenderRect rc{0, 0, 0, 0};  // empty for everything off the image, for non-finite positions and for the lanes past the end
    float2 p = make_float2(0.0f, 0.0f);
    if (live) {
        p = pos[j];
        rc = render_pixel_rect(v, p.x, p.y);
    }
    const uint32_t mine = FLUID ? 2u + j : 1u;
    const uint32_t w = rc.x1 - rc.x0, h = rc.y1 - rc.y0;
    if (__any(w > RENDER_COMBINE || h > RENDER_COMBINE)) {
        for (uint32_t iy = rc.y0; iy < rc.y1; ++iy) {
            const float qy = render_qy(v, iy);
            uint32_t* const row = code + (size_t)iy * v.width;
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
            seen[dy * RENDER_COMBINE + dx] = cov ? __atomic_load_n(code + ((rc.y0 + dy) * v.width + rc.x0 + dx), __ATOMIC_RELAXED) : 0xFFFFFFFFu;
        }
    }
#pragma unroll
    for (uint32_t dy = 0; dy < RENDER_COMBINE; ++dy) {
#pragma unroll
        for (uint32_t dx = 0; dx < RENDER_COMBINE; ++dx) {
            const bool need = seen[dy * RENDER_COMBINE + dx] < mine;  // (not covered: 0xFFFFFFFF, never below a code)
            const uint32_t key = need ? (rc.y0 + dy) * v.width + rc.x0 + dx : 0xFFFFFFFFu;  // (< 2^28 for a pixel of the image)
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
            hipLaunchKernelGGL(k_render_scatter<false>, dim3(nb), dim3(256), 0, st, (const float2*)c->bpos, c->B, v, code, base);
        });
    if (c->N)
        render_pieces(c, "render_scatter", 8.0 * c->N, c->N, [&](uint32_t nb, uint32_t base) {
            hipLaunchKernelGGL(k_render_scatter<true>, dim3(nb), dim3(256), 0, st, (const float2*)c->posA, c->N, v, code, base);
        });
    render_pieces(c, "render_resolve", (4.0 + (rgba ? 4.0 : 0.0) + (owner ? 4.0 : 0.0)) * npix, npix, [&](uint32_t nb, uint32_t base) {
        hipLaunchKernelGGL(k_render_resolve, dim3(nb), dim3(256), 0, st, (const uint32_t*)code, (const float2*)c->vel, npix, view.speed_scale,
                           pack_rgba(view.background), pack_rgba(view.boundary), rgba, owner, base);
    });
    c->K.rev = rev;
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
    if (!std::isfinite(view->pixel_per_world_unit) || !(view->pixel_per_world_unit > 0.0f))
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_render: view.pixel_per_world_unit must be finite and > 0");
    if (!std::isfinite(view->center[0]) || !std::isfinite(view->center[1])) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_render: view.center must be finite");
    if (!std::isfinite(view->radius) || view->radius < 0.0f || view->radius > c->P.smoothing_length)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_render: view.radius must be finite and in [0, smoothing_length]");
    if (!std::isfinite(view->min_pixel_radius) || view->min_pixel_radius < 0.0f || view->min_pixel_radius > 4.0f)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_render: view.min_pixel_radius must be finite and in [0, 4]");
    if (!std::isfinite(view->speed_scale)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_render: view.speed_scale must be finite");
    const uint64_t npix = (uint64_t)view->width * view->height;
    if (npix >= (1ull << 28)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_render: view.width * view.height must be < 2^28");
    if (c->N > 0xFFFFFFFDu) return c->fail(SPHX_ERR_CAPACITY, "sphx_render: more than 2^32 - 3 particles (two owner codes are taken)");
    if (npix == 0) return SPHX_OK;
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, "sphx_render: between step_begin and step_finish (finish the step first)");
    SPHX_HIP(c, hipSetDevice(c->device));
    flush_pending_advect(c);

    RenderCam v;
    v.cx = view->center[0], v.cy = view->center[1];
    v.ppu = view->pixel_per_world_unit;
    v.inv = 1.0f / view->pixel_per_world_unit;
    const float r_world = view->radius > 0.0f ? view->radius : c->P.particle_radius, r_pixel = view->min_pixel_radius * v.inv;
    v.r = r_world > r_pixel ? r_world : r_pixel;
    v.r2 = v.r * v.r;
    v.width = view->width, v.height = view->height;

    // scratch: the owner codes, and on the host-pointer path the device copies of the outputs behind them
    const bool dev = flags & SPHX_RENDER_DEVICE_POINTERS;
    const size_t need = (size_t)npix * (1u + (!dev && out->rgba ? 1u : 0u) + (!dev && out->owner ? 1u : 0u));
    if (need > c->render_cap) {
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
        int rc;
        if ((rc = dev_alloc(c, &c->render_buf, need))) {
            c->render_cap = 0;
            return rc;
        }
        c->render_cap = need;
    }
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

}  // extern "C"
