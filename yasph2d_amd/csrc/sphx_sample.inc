// sphx_sample.inc — field sampling at arbitrary points and on a regular lattice (sphx_sample_points / sphx_sample_grid, include/sphx.h):
// the kernel interpolation an SPH "measure tool" does, over the cell grids the latest neighbour build left on the device.
// Included at the end of sphx_kernels.hip (one translation unit: cell_of, slots9n, ranges9n, gat, the kernel evaluators, NbGrid and the
// launch layer of sphx_launch.inc are visible).  Compiled with -ffp-contract=off like the rest: the fp32 expressions below are the
// contract of sphx.h, restated bit for bit by tests/sample_reference.py.

namespace sphx {

// The arrays sphx_download copies (after the step's pointer swaps) and the two grids of the latest build.
struct SampleArgs {
    const float2* pos;     // posA: [N|B] positions, boundary records at soff + j
    const float2* vel;     // [N] velocities
    const float* density;  // [N] the solver's densities
    uint32_t soff;
    NbGrid gd, gs;         // dynamic and static grid (nview)
    float* o_density;      // [m] or null
    float* o_fraction;     // [m] or null
    float* o_velocity;     // [2m] interleaved, or null
    uint32_t* o_count;     // [m] or null
};
// lattice point (ix, iy) = (x0 + (float)ix * dx, y0 + (float)iy * dy); a workgroup covers 16 x 16 points, each wavefront 8 x 8 of them
struct SampleLattice {
    float x0, y0, dx, dy;
    uint32_t nx, ny, tiles_x;  // tiles_x = ceil(nx / 16)
};
constexpr uint32_t SAMPLE_TILE = 16;             // lattice points per workgroup side
constexpr uint32_t SAMPLE_MAX_BLOCKS = 1u << 22;  // workgroups per launch (2^30 work-items: the 32-bit grid size of a dispatch)

// W(d2) of the kernel kind, as sphx_update_densities evaluates it.  sqrtf, not sqrt_dist: a query point may sit exactly on a particle
// (d2 = 0 is accepted here, never in a neighbour build), where the FAST form's rsq(0) = inf gives NaN.
template <int KIND>
__device__ __forceinline__ float sample_w(const Consts& K, float d2) {
    if (KIND == SPHX_KERNEL_POLY6) return poly6_eval(K, d2);
    const float r = sqrtf(d2);
    if (KIND == SPHX_KERNEL_WENDLAND_C2) return wendland_eval(K, r);
    return spiky_eval(K, r);
}

// The walk of ONE query point (both paths; a lane per point).  DEN: density (fluid, then boundary); FRAC: the a_j = (m / rho_j) w sums
// (fraction or velocity requested: loads density[]); VEL: the a_j v_j sums (loads vel[]).  The count is always formed (an integer add
// per accepted candidate).  Candidates: the fluid particles of the 3 x 3 cells around cell_of(q) in ascending slot order (slots9n sorts
// the box's cells by table slot, so the ranges follow each other in ascending particle index), then the boundary particles of those
// cells in the same order.  A dead lane (live = false) takes part in the wavefront's directory look-ups and walks nothing.
struct SampleSums {
    float rho, frac, svx, svy;  // density; sum a_j; sum a_j v_j (not yet divided)
    uint32_t cnt;
};
template <int KIND, bool DEN, bool FRAC, bool VEL>
__device__ __forceinline__ SampleSums sample_walk(const Consts& K, const SampleArgs& a, float qx, float qy, bool live) {
    uint32_t cx, cy;
    cell_of(K, make_float2(qx, qy), cx, cy);  // a NaN coordinate saturates to cell 0, and every distance test with it fails
    uint32_t slot[9], s[9], e[9], centre, any9;
    slots9n(a.gd, cx, cy, slot, centre, any9);
    ranges9n(a.gd, slot, s, e);
    float rho = 0.0f, frac = 0.0f, svx = 0.0f, svy = 0.0f;
    uint32_t cnt = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const uint32_t end = live ? e[t] : s[t];
        for (uint32_t j = s[t]; j < end; ++j) {
            const float2 pj = gat(a.pos, j);
            const float dx = pj.x - qx, dy = pj.y - qy;
            const float d2 = dx * dx + dy * dy;
            if (d2 <= K.radius_sq) {  // (no d2 > 1e-10 exclusion: a query point is not a particle)
                cnt += 1u;
                if (DEN || FRAC) {
                    const float w = sample_w<KIND>(K, d2);
                    if (DEN) rho = rho + w * K.mass;
                    if (FRAC) {
                        const float aj = (K.mass / gat(a.density, j)) * w;
                        frac = frac + aj;
                        if (VEL) {
                            const float2 vj = gat(a.vel, j);
                            svx = svx + aj * vj.x;
                            svy = svy + aj * vj.y;
                        }
                    }
                }
            }
        }
    }
    if (DEN) {
        // boundary particles: only where the box can hold some — the build's gate (k_neighbor_build): the dynamic directory's DIRN_FLAG of
        // the box's own block, or a block outside the dynamic directory's rectangle (its look-up was clamped), then the static grid's
        // DIRN_FLAG of the nine cells.  Per lane here: a lane the gate excludes has no boundary particle in its box.
        const bool maybe_static = live && ((centre & DIRN_FLAG) != 0u || (cx >> BLOCK_SHIFT) - a.gd.bx0 > a.gd.nbx1 ||
                                           (cy >> BLOCK_SHIFT) - a.gd.by0 > a.gd.nby1);
        if (__any(maybe_static)) {
            slots9n(a.gs, cx, cy, slot, centre, any9);
            const bool walk = maybe_static && (any9 & DIRN_FLAG) != 0u;
            if (__any(walk)) {
                ranges9n(a.gs, slot, s, e);
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const uint32_t end = walk ? e[t] : s[t];
                    for (uint32_t j = s[t]; j < end; ++j) {
                        const float2 pj = gat(a.pos, a.soff + j);
                        const float dx = pj.x - qx, dy = pj.y - qy;
                        const float d2 = dx * dx + dy * dy;
                        if (d2 <= K.radius_sq) rho = rho + sample_w<KIND>(K, d2) * K.mass;
                    }
                }
            }
        }
    }
    return SampleSums{rho, frac, svx, svy, cnt};
}
// Shepard-normalised velocity; (0, 0) where no fluid particle contributes
__device__ __forceinline__ float2 sample_velocity(const SampleSums& r) {
    const bool some = r.frac != 0.0f;
    return make_float2(some ? r.svx / r.frac : 0.0f, some ? r.svy / r.frac : 0.0f);
}
// ... and its outputs into the arrays of SampleArgs at index o
template <int KIND, bool DEN, bool FRAC, bool VEL>
__device__ __forceinline__ void sample_point(const Consts& K, const SampleArgs& a, float qx, float qy, bool live, uint32_t o) {
    const SampleSums r = sample_walk<KIND, DEN, FRAC, VEL>(K, a, qx, qy, live);
    if (!live) return;
    if (DEN && a.o_density) a.o_density[o] = r.rho;
    if (FRAC && a.o_fraction) a.o_fraction[o] = r.frac;
    if (VEL && a.o_velocity) {
        const float2 v = sample_velocity(r);
        a.o_velocity[2 * (size_t)o] = v.x;
        a.o_velocity[2 * (size_t)o + 1] = v.y;
    }
    if (a.o_count) a.o_count[o] = r.cnt;
}

// point path: point base + blockIdx.x * 256 + threadIdx.x of xy[] (caller order — sphx.h asks for spatially coherent point sets)
template <int KIND, bool DEN, bool FRAC, bool VEL>
__global__ __launch_bounds__(256) void k_sample_points(Consts K, SampleArgs a, const float* __restrict__ xy, uint32_t m, uint32_t base) {
    const uint32_t i = base + blockIdx.x * 256u + threadIdx.x;
    const bool live = i < m;
    const uint32_t k = live ? i : m - 1u;  // (m > 0: the host launches nothing for an empty set)
    sample_point<KIND, DEN, FRAC, VEL>(K, a, xy[2 * (size_t)k], xy[2 * (size_t)k + 1], live, k);
}

// lattice path: workgroup base + blockIdx.x covers lattice tile (tx, ty) of 16 x 16 points, wavefront w its 8 x 8 quarter
// (w & 1, w >> 1), lane l the point (l & 7, l >> 3) of it: the 3 x 3 boxes of a wavefront's lanes overlap, their gathers share lines.
template <int KIND, bool DEN, bool FRAC, bool VEL>
__global__ __launch_bounds__(256) void k_sample_grid(Consts K, SampleArgs a, SampleLattice L, uint32_t base) {
    const uint32_t b = base + blockIdx.x;
    const uint32_t ty = b / L.tiles_x, tx = b - ty * L.tiles_x;
    const uint32_t w = threadIdx.x >> 6, l = threadIdx.x & 63u;
    const uint32_t ix = tx * SAMPLE_TILE + (w & 1u) * 8u + (l & 7u), iy = ty * SAMPLE_TILE + (w >> 1) * 8u + (l >> 3);
    const bool live = ix < L.nx && iy < L.ny;
    const uint32_t jx = min(ix, L.nx - 1u), jy = min(iy, L.ny - 1u);  // (a dead lane walks nothing; its point stays next to its wavefront's)
    const float qx = L.x0 + (float)jx * L.dx;
    const float qy = L.y0 + (float)jy * L.dy;
    sample_point<KIND, DEN, FRAC, VEL>(K, a, qx, qy, live, jy * L.nx + jx);
}

// ---- one tile of a tiled run (sphx_tile_sample_points / _window, include/sphx.h "sampling the fields of a tiled run") -------------------
// A tile answers the points whose cell lies in its owned rectangle K.tile; the walk is sample_walk over the tile's own arrays.

// points, pass 1: the indices of the points this tile owns, appended behind head[0].  A wavefront reserves its entries with ONE atomic
// (ballot, population count, lane 0 adds, prefix of the ballot per lane — the scheme of k_track_window_owned); the loop bounds are
// workgroup-uniform, so all 64 lanes are active at the ballot.  The list holds m entries and a point is appended at most once: it
// cannot overflow.  Its order is whatever the atomics give; pass 2 carries the index along and the host scatters by it.
__global__ __launch_bounds__(256) void k_tile_sample_select(Consts K, const float2* __restrict__ xy, uint32_t m, uint32_t* __restrict__ head,
                                                            uint32_t* __restrict__ list) {
    const uint32_t chunks = (m + 255u) / 256u;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const uint32_t i = ch * 256u + threadIdx.x;
        bool own = false;
        if (i < m) {
            uint32_t cx, cy;
            cell_of(K, xy[i], cx, cy);
            own = rect_has(K.tile, cx, cy, 0u);
        }
        const unsigned long long b = __ballot(own);
        if (!b) continue;  // (wave-uniform)
        uint32_t base = 0;
        if (lane == 0u) base = atomicAdd(head, (uint32_t)__popcll(b));
        base = __shfl(base, 0);
        if (own) list[base + (uint32_t)__popcll(b & below)] = i;
    }
}

// points, pass 2: entry k of the list -> one packed 24-byte record {index, density, fraction, vx, vy, count} (a field that was not asked
// for is stored as zero).  The number of entries is read from head[0]: the launch is sized for m and the workgroups beyond the list
// leave at once, so no host round trip separates the passes.  Every lane of a wavefront inside the list is live.
template <int KIND, bool DEN, bool FRAC, bool VEL>
__global__ __launch_bounds__(256) void k_tile_sample_indexed(Consts K, SampleArgs a, const float2* __restrict__ xy, const uint32_t* __restrict__ head,
                                                             const uint32_t* __restrict__ list, uint2* __restrict__ rec) {
    const uint32_t n = head[0];
    const uint32_t chunks = (n + 255u) / 256u;
    for (uint32_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const uint32_t k = ch * 256u + threadIdx.x;
        const bool live = k < n;
        const uint32_t i = list[live ? k : n - 1u];  // (n > 0 inside the loop; a dead lane stays next to its wavefront's points)
        const float2 q = xy[i];
        const SampleSums r = sample_walk<KIND, DEN, FRAC, VEL>(K, a, q.x, q.y, live);
        if (!live) continue;
        const float2 v = VEL ? sample_velocity(r) : make_float2(0.0f, 0.0f);
        rec[3 * (size_t)k] = make_uint2(i, DEN ? __float_as_uint(r.rho) : 0u);
        rec[3 * (size_t)k + 1] = make_uint2(FRAC ? __float_as_uint(r.frac) : 0u, __float_as_uint(v.x));
        rec[3 * (size_t)k + 2] = make_uint2(__float_as_uint(v.y), r.cnt);
    }
}

// lattice: k_sample_grid over the window [ix0, ix0 + wnx) x [iy0, iy0 + wny) of the lattice L — the index rectangle of the points this
// tile owns (sphx_sample_window.hpp).  The point is formed from the GLOBAL index; the outputs go to window-sized arrays, row after row
// (W.pitch words apart).
// A lane whose cell is not the tile's writes nothing (the host's window holds no such lane; the buffers are zeroed before the launch).
struct SampleWindow {
    uint32_t ix0, iy0, wnx, wny, tiles_x;  // tiles_x = ceil(wnx / 16)
    uint32_t pitch;                        // words per output row: wnx, or wnx + 1 where the contour keeps an apron column behind it
};
template <int KIND, bool DEN, bool FRAC, bool VEL>
__global__ __launch_bounds__(256) void k_tile_sample_window(Consts K, SampleArgs a, SampleLattice L, SampleWindow W, uint32_t base) {
    const uint32_t b = base + blockIdx.x;
    const uint32_t ty = b / W.tiles_x, tx = b - ty * W.tiles_x;
    const uint32_t w = threadIdx.x >> 6, l = threadIdx.x & 63u;
    const uint32_t lx = tx * SAMPLE_TILE + (w & 1u) * 8u + (l & 7u), ly = ty * SAMPLE_TILE + (w >> 1) * 8u + (l >> 3);
    const bool inside = lx < W.wnx && ly < W.wny;
    const uint32_t jx = min(lx, W.wnx - 1u), jy = min(ly, W.wny - 1u);
    const float qx = L.x0 + (float)(W.ix0 + jx) * L.dx;
    const float qy = L.y0 + (float)(W.iy0 + jy) * L.dy;
    uint32_t cx, cy;
    cell_of(K, make_float2(qx, qy), cx, cy);
    sample_point<KIND, DEN, FRAC, VEL>(K, a, qx, qy, inside && rect_has(K.tile, cx, cy, 0u), jy * W.pitch + jx);
}

}  // namespace sphx

// ---- launch layer and C ABI ----------------------------------------------------------------------------------------------------------
namespace {

constexpr uint32_t SAMPLE_OUT_DENSITY = 1u, SAMPLE_OUT_FRACTION = 2u, SAMPLE_OUT_VELOCITY = 4u, SAMPLE_OUT_COUNT = 8u;

// one query: either m points at xy (device pointer) or the lattice L
struct SampleJob {
    const float* xy;
    uint32_t m;
    const SampleLattice* lattice;
    SampleArgs a;
    // a tile's query (sphx_tile_sample_*): the window of the lattice, or the list of owned points and their records
    const SampleWindow* window = nullptr;
    const uint32_t* head = nullptr;
    const uint32_t* list = nullptr;
    uint2* rec = nullptr;
};

template <int KIND, bool DEN, bool FRAC, bool VEL>
void enqueue_sample_t(sphx_ctx* c, const SampleJob& q, uint64_t points) {
    // algorithmic bytes: the point (8, points path), the outputs, and ~ (9 cells) x (8-byte table entry) + the accepted records
    const double per = (q.lattice ? 0.0 : 8.0) + (DEN ? 4 : 0) + (FRAC ? 4 : 0) + (VEL ? 8 : 0) + 4 + 72.0;
    const uint32_t rev = c->K.rev;  // (a query must not change the sweep direction of the step's next kernels: launch() toggles it)
    hipStream_t st = c->stream;
    if (q.rec) {
        // (sized for all m points: the workgroups beyond the tile's list read its length and leave)
        const uint32_t nb = (uint32_t)std::min<uint64_t>(((uint64_t)q.m + 255u) / 256u, SAMPLE_MAX_BLOCKS);
        launch(c, "tile_sample_indexed", (per + 4.0 + 24.0) * (double)points, [&] {
            hipLaunchKernelGGL((k_tile_sample_indexed<KIND, DEN, FRAC, VEL>), dim3(nb), dim3(256), 0, st, c->K, q.a, (const float2*)q.xy, q.head, q.list, q.rec);
        });
    } else if (q.window) {
        const SampleLattice L = *q.lattice;
        const SampleWindow W = *q.window;
        const uint64_t blocks = (uint64_t)W.tiles_x * ((W.wny + SAMPLE_TILE - 1) / SAMPLE_TILE);
        for (uint64_t b0 = 0; b0 < blocks; b0 += SAMPLE_MAX_BLOCKS) {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(blocks - b0, SAMPLE_MAX_BLOCKS);
            launch(c, "tile_sample_window", per * (double)points * nb / (double)blocks, [&] {
                hipLaunchKernelGGL((k_tile_sample_window<KIND, DEN, FRAC, VEL>), dim3(nb), dim3(256), 0, st, c->K, q.a, L, W, (uint32_t)b0);
            });
        }
    } else if (q.lattice) {
        const SampleLattice L = *q.lattice;
        const uint64_t blocks = (uint64_t)L.tiles_x * ((L.ny + SAMPLE_TILE - 1) / SAMPLE_TILE);
        for (uint64_t b0 = 0; b0 < blocks; b0 += SAMPLE_MAX_BLOCKS) {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(blocks - b0, SAMPLE_MAX_BLOCKS);
            launch(c, "sample_grid", per * (double)points * nb / (double)blocks, [&] {
                hipLaunchKernelGGL((k_sample_grid<KIND, DEN, FRAC, VEL>), dim3(nb), dim3(256), 0, st, c->K, q.a, L, (uint32_t)b0);
            });
        }
    } else {
        const uint64_t blocks = ((uint64_t)q.m + 255u) / 256u;
        for (uint64_t b0 = 0; b0 < blocks; b0 += SAMPLE_MAX_BLOCKS) {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(blocks - b0, SAMPLE_MAX_BLOCKS);
            launch(c, "sample_points", per * (double)points * nb / (double)blocks, [&] {
                hipLaunchKernelGGL((k_sample_points<KIND, DEN, FRAC, VEL>), dim3(nb), dim3(256), 0, st, c->K, q.a, q.xy, q.m, (uint32_t)(b0 * 256u));
            });
        }
    }
    c->K.rev = rev;
}

template <int KIND>
void enqueue_sample_k(sphx_ctx* c, const SampleJob& q, uint32_t outs, uint64_t points) {
    const bool den = outs & SAMPLE_OUT_DENSITY, vel = outs & SAMPLE_OUT_VELOCITY, frac = vel || (outs & SAMPLE_OUT_FRACTION);
    if (den && frac && vel) enqueue_sample_t<KIND, true, true, true>(c, q, points);
    else if (den && frac) enqueue_sample_t<KIND, true, true, false>(c, q, points);
    else if (den) enqueue_sample_t<KIND, true, false, false>(c, q, points);
    else if (vel) enqueue_sample_t<KIND, false, true, true>(c, q, points);
    else if (frac) enqueue_sample_t<KIND, false, true, false>(c, q, points);
    else enqueue_sample_t<SPHX_KERNEL_WENDLAND_C2, false, false, false>(c, q, points);  // count only: no kernel evaluated
}

void enqueue_sample(sphx_ctx* c, const SampleJob& q, int kind, uint32_t outs, uint64_t points) {
    if (kind == SPHX_KERNEL_WENDLAND_C2) enqueue_sample_k<SPHX_KERNEL_WENDLAND_C2>(c, q, outs, points);
    else if (kind == SPHX_KERNEL_POLY6) enqueue_sample_k<SPHX_KERNEL_POLY6>(c, q, outs, points);
    else enqueue_sample_k<SPHX_KERNEL_SPIKY>(c, q, outs, points);
}

uint32_t sample_outputs(const sphx_sample_out* out) {
    return (out->density ? SAMPLE_OUT_DENSITY : 0u) | (out->fraction ? SAMPLE_OUT_FRACTION : 0u) | (out->velocity ? SAMPLE_OUT_VELOCITY : 0u) |
           (out->count ? SAMPLE_OUT_COUNT : 0u);
}

// the argument checks both calls share (they name the argument; a tile context is refused as an argument)
int sample_check_args(sphx_ctx* c, const char* fn, int kind, uint32_t flags, const sphx_sample_out* out) {
    const std::string f = fn;
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": out is NULL").c_str());
    if (!sample_outputs(out)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": out requests no output (every pointer is NULL)").c_str());
    if (kind != SPHX_KERNEL_WENDLAND_C2 && kind != SPHX_KERNEL_POLY6 && kind != SPHX_KERNEL_SPIKY)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": unknown kernel_kind").c_str());
    if (flags & ~(uint32_t)SPHX_SAMPLE_DEVICE_POINTERS) return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": unknown flags bits").c_str());
    if (c->tile_mode)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": not available on a tile context (its arrays hold ghosts and miss the particles other tiles own)").c_str());
    return SPHX_OK;
}

// the state a query needs: not inside a step, cell grids and densities of the current positions (sphx_ctx::sample_ready)
int sample_check_state(sphx_ctx* c, const char* fn) {
    const std::string f = fn;
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, (f + ": between step_begin and step_finish (finish the step first)").c_str());
    if (!c->uploaded) return c->fail(SPHX_ERR_NOT_READY, (f + ": no particles uploaded").c_str());
    if (c->sample_ready != 2u) return c->fail(SPHX_ERR_NOT_READY, (f + ": " + c->sample_missing).c_str());
    return SPHX_OK;
}

SampleArgs sample_args(const sphx_ctx* c, const sphx_sample_out& o) {
    return SampleArgs{(const float2*)c->posA, (const float2*)c->vel, (const float*)c->density, c->soff(), c->gdyn.nview(), c->gstat.nview(),
                      o.density, o.fraction, o.velocity, o.count};
}

// host pointers: the query runs on device copies in the context's scratch (grown on demand), the outputs come back before the return
int sample_host(sphx_ctx* c, const float* xy, uint64_t m, const SampleLattice* L, int kind, const sphx_sample_out& out) {
    const uint32_t outs = sample_outputs(&out);
    const size_t n_xy = L ? 0 : 2 * m, n_d = out.density ? m : 0, n_f = out.fraction ? m : 0, n_v = out.velocity ? 2 * m : 0,
                 n_c = out.count ? m : 0;
    const size_t need = n_xy + n_d + n_f + n_v + n_c;  // 4-byte words
    if (need > c->sample_cap) {
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
        int rc;
        if ((rc = dev_alloc(c, &c->sample_buf, need))) {
            c->sample_cap = 0;
            return rc;
        }
        c->sample_cap = need;
    }
    float* p = c->sample_buf;
    float* d_xy = p;
    p += n_xy;
    sphx_sample_out dev{};
    dev.density = out.density ? p : nullptr;
    p += n_d;
    dev.fraction = out.fraction ? p : nullptr;
    p += n_f;
    dev.velocity = out.velocity ? p : nullptr;
    p += n_v;
    dev.count = out.count ? (uint32_t*)p : nullptr;
    if (n_xy) SPHX_HIP(c, hipMemcpyAsync(d_xy, xy, n_xy * 4, hipMemcpyHostToDevice, c->stream));
    enqueue_sample(c, SampleJob{d_xy, (uint32_t)m, L, sample_args(c, dev)}, kind, outs, m);
    if (n_d) SPHX_HIP(c, hipMemcpyAsync(out.density, dev.density, n_d * 4, hipMemcpyDeviceToHost, c->stream));
    if (n_f) SPHX_HIP(c, hipMemcpyAsync(out.fraction, dev.fraction, n_f * 4, hipMemcpyDeviceToHost, c->stream));
    if (n_v) SPHX_HIP(c, hipMemcpyAsync(out.velocity, dev.velocity, n_v * 4, hipMemcpyDeviceToHost, c->stream));
    if (n_c) SPHX_HIP(c, hipMemcpyAsync(out.count, dev.count, n_c * 4, hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    return SPHX_OK;
}

}  // namespace

extern "C" {

int sphx_sample_points(sphx_ctx* c, const float* xy, uint32_t m, int kernel_kind, uint32_t flags, const sphx_sample_out* out) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = sample_check_args(c, "sphx_sample_points", kernel_kind, flags, out))) return rc;
    if (m && !xy) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_sample_points: xy is NULL with m > 0");
    if (m == 0) return SPHX_OK;
    if ((rc = sample_check_state(c, "sphx_sample_points"))) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    if (flags & SPHX_SAMPLE_DEVICE_POINTERS) {
        enqueue_sample(c, SampleJob{xy, m, nullptr, sample_args(c, *out)}, kernel_kind, sample_outputs(out), m);
        return SPHX_OK;
    }
    return sample_host(c, xy, m, nullptr, kernel_kind, *out);
}

int sphx_sample_grid(sphx_ctx* c, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, int kernel_kind, uint32_t flags,
                     const sphx_sample_out* out) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = sample_check_args(c, "sphx_sample_grid", kernel_kind, flags, out))) return rc;
    if (!std::isfinite(x0) || !std::isfinite(y0)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_sample_grid: x0 / y0 must be finite");
    if (!std::isfinite(dx) || !(dx > 0.0f)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_sample_grid: dx must be finite and > 0");
    if (!std::isfinite(dy) || !(dy > 0.0f)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_sample_grid: dy must be finite and > 0");
    const uint64_t m = (uint64_t)nx * ny;
    if (m >= (1ull << 31)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_sample_grid: nx * ny must be < 2^31");
    if (m == 0) return SPHX_OK;
    if ((rc = sample_check_state(c, "sphx_sample_grid"))) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    const SampleLattice L{x0, y0, dx, dy, nx, ny, (nx + SAMPLE_TILE - 1) / SAMPLE_TILE};
    if (flags & SPHX_SAMPLE_DEVICE_POINTERS) {
        enqueue_sample(c, SampleJob{nullptr, 0, &L, sample_args(c, *out)}, kernel_kind, sample_outputs(out), m);
        return SPHX_OK;
    }
    return sample_host(c, nullptr, m, &L, kernel_kind, *out);
}

}  // extern "C"

// ---- one tile of a tiled run: the seam sphx_multi_sample_points / _grid (sphx_tiles.cpp) are built on ---------------------------------
// Enqueue and fetch halves, like the render and statistics seams: the multi enqueues on every tile's stream first and then collects, so
// the tiles' passes overlap.  The scratch is sample_buf (sphx_sample_* refuse a tile context, so nobody else uses it there).
#include "sphx_sample_window.hpp"

namespace {

static_assert(SPHX_SAMPLE_FIELD_DENSITY == SAMPLE_OUT_DENSITY && SPHX_SAMPLE_FIELD_FRACTION == SAMPLE_OUT_FRACTION &&
                  SPHX_SAMPLE_FIELD_VELOCITY == SAMPLE_OUT_VELOCITY && SPHX_SAMPLE_FIELD_COUNT == SAMPLE_OUT_COUNT,
              "the field bits of the tile seam are the launch layer's output bits");
constexpr uint32_t SAMPLE_FIELDS_ALL = SAMPLE_OUT_DENSITY | SAMPLE_OUT_FRACTION | SAMPLE_OUT_VELOCITY | SAMPLE_OUT_COUNT;
constexpr size_t SAMPLE_HEAD_WORDS = 4;    // the list's counter, 16 bytes: what follows stays 8-byte aligned
constexpr size_t SAMPLE_RECORD_WORDS = 6;  // {index, density, fraction, vx, vy, count}

int tile_sample_check(sphx_ctx* c, const char* fn, int kind, uint32_t fields) {
    const std::string f = fn;
    if (!c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": not a tile context (sphx_sample_points / sphx_sample_grid serve a plain one)").c_str());
    if (!fields) return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": fields requests no output").c_str());
    if (fields & ~SAMPLE_FIELDS_ALL) return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": unknown fields bits").c_str());
    if (kind != SPHX_KERNEL_WENDLAND_C2 && kind != SPHX_KERNEL_POLY6 && kind != SPHX_KERNEL_SPIKY)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": unknown kernel_kind").c_str());
    return SPHX_OK;
}
// the state a tile's query needs: the re-grid after the latest halo exchange has run (cell grids, density[] and the static grid belong
// to the positions; an empty tile's re-grid says so too) and no step is open
int tile_sample_state(sphx_ctx* c, const char* fn) {
    const std::string f = fn;
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, (f + ": between step_begin and step_finish (finish the step first)").c_str());
    if (!c->lists_current || c->tile_pending_dt > 0.0f || !c->tile_density_ready || c->boundary_changed)
        return c->fail(SPHX_ERR_NOT_READY, (f + ": the tile is between a halo exchange and its re-grid (sphx_sub_regrid first)").c_str());
    return SPHX_OK;
}
int tile_sample_scratch(sphx_ctx* c, size_t words) {
    if (words <= c->sample_cap && c->sample_buf) return SPHX_OK;
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    int rc;
    if ((rc = dev_alloc(c, &c->sample_buf, words))) {
        c->sample_cap = 0;
        return rc;
    }
    c->sample_cap = words;
    return SPHX_OK;
}
// The grids a tile's walk reads.  A tile that holds no particle at all (N == 0: it owns cells, perhaps walls, and no fluid, and no ghost
// has reached it) may never have built a dynamic grid: it walks the NULL GRID instead — one directory entry that points at BLOCK_CELLS
// empty ranges and carries DIRN_FLAG, as the null entries of a real dynamic directory do, so the boundary walk stays open and the tile
// answers from its static grid alone.  A context without a static grid gets the unflagged twin.
int tile_sample_grids(sphx_ctx* c, NbGrid& gd, NbGrid& gs) {
    const bool dyn = c->N && c->gdyn.dirn && c->gdyn.fine, stat = c->gstat.dirn && c->gstat.fine;
    if ((!dyn || !stat) && !c->tsample.null_grid) {
        static const uint32_t entries[2] = {DIRN_FLAG, 0u};
        int rc;
        if ((rc = dev_alloc(c, &c->tsample.null_grid, 2 * (size_t)BLOCK_CELLS + 2))) return rc;
        SPHX_HIP(c, hipMemsetAsync(c->tsample.null_grid, 0, 2 * (size_t)BLOCK_CELLS * 4, c->stream));
        SPHX_HIP(c, hipMemcpyAsync(c->tsample.null_grid + 2 * (size_t)BLOCK_CELLS, entries, sizeof(entries), hipMemcpyHostToDevice, c->stream));
    }
    const uint32_t* const ng = c->tsample.null_grid;
    gd = dyn ? c->gdyn.nview() : NbGrid{ng + 2 * (size_t)BLOCK_CELLS, (const uint2*)ng, 0u, 0u, 1u, 0u, 0u};
    gs = stat ? c->gstat.nview() : NbGrid{ng + 2 * (size_t)BLOCK_CELLS + 1, (const uint2*)ng, 0u, 0u, 1u, 0u, 0u};
    return SPHX_OK;
}

}  // namespace

extern "C" {

int sphx_tile_sample_points(sphx_ctx* c, const float* xy, uint32_t m, int kernel_kind, uint32_t fields) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_sample_points";
    int rc;
    if ((rc = tile_sample_check(c, fn, kernel_kind, fields))) return rc;
    if (m && !xy) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_sample_points: xy is NULL with m > 0");
    if (m >= (1u << 31)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_sample_points: m must be < 2^31");
    c->tsample.m = 0;
    if (m == 0) return SPHX_OK;
    if ((rc = tile_sample_state(c, fn))) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    // scratch: counter | points [2m] | list [m, rounded up to even] | records [6m]
    const size_t at_xy = SAMPLE_HEAD_WORDS, at_list = at_xy + 2 * (size_t)m, at_rec = at_list + (((size_t)m + 1u) & ~(size_t)1u);
    if ((rc = tile_sample_scratch(c, at_rec + SAMPLE_RECORD_WORDS * (size_t)m))) return rc;
    SampleArgs a{(const float2*)c->posA, (const float2*)c->vel, (const float*)c->density, c->soff(), NbGrid{}, NbGrid{}, nullptr, nullptr, nullptr, nullptr};
    if ((rc = tile_sample_grids(c, a.gd, a.gs))) return rc;
    uint32_t* const buf = (uint32_t*)c->sample_buf;
    hipStream_t st = c->stream;
    SPHX_HIP(c, hipMemsetAsync(buf, 0, SAMPLE_HEAD_WORDS * 4, st));
    SPHX_HIP(c, hipMemcpyAsync(buf + at_xy, xy, 2 * (size_t)m * 4, hipMemcpyHostToDevice, st));
    const uint32_t rev = c->K.rev;  // (launch() toggles the sweep direction of the step's next kernels: put back below)
    const uint32_t nb = (uint32_t)std::min<uint64_t>(((uint64_t)m + 255u) / 256u, SAMPLE_MAX_BLOCKS);
    launch(c, "tile_sample_select", 12.0 * m, [&] {
        hipLaunchKernelGGL(k_tile_sample_select, dim3(nb), dim3(256), 0, st, c->K, (const float2*)(buf + at_xy), m, buf, buf + at_list);
    });
    SampleJob q{(const float*)(buf + at_xy), m, nullptr, a};
    q.head = buf;
    q.list = buf + at_list;
    q.rec = (uint2*)(buf + at_rec);
    enqueue_sample(c, q, kernel_kind, fields, m);
    c->K.rev = rev;
    c->tsample.m = m;
    c->tsample.fields = fields;
    c->tsample.rec_at = at_rec;
    return SPHX_OK;
}

int sphx_tile_sample_points_fetch(sphx_ctx* c, uint32_t* records, uint32_t cap_records, uint32_t* out_n) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_sample_points_fetch";
    if (!out_n || (cap_records && !records)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "records or out_n is NULL");
    *out_n = 0;
    if (!c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not a tile context");
    const uint32_t m = c->tsample.m;
    if (!m) return SPHX_OK;  // (an empty query, or none: nothing was queued)
    c->tsample.m = 0;
    SPHX_HIP(c, hipSetDevice(c->device));
    uint32_t n = 0;
    SPHX_HIP(c, hipMemcpyAsync(&n, c->sample_buf, 4, hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    if (n > m) return c->fail(SPHX_ERR_HIP, fn, "the list of owned points is longer than the point set");
    if (n > cap_records) return c->fail(SPHX_ERR_CAPACITY, fn, "the tile answers more points than cap_records");
    if (n) {
        SPHX_HIP(c, hipMemcpyAsync(records, (const uint32_t*)c->sample_buf + c->tsample.rec_at, (size_t)n * SAMPLE_RECORD_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
    }
    *out_n = n;
    return SPHX_OK;
}

int sphx_tile_sample_window(sphx_ctx* c, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, int kernel_kind, uint32_t fields,
                            uint32_t* out_window) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_sample_window";
    if (!out_window) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out_window is NULL");
    out_window[0] = out_window[1] = out_window[2] = out_window[3] = 0u;
    int rc;
    if ((rc = tile_sample_check(c, fn, kernel_kind, fields))) return rc;
    if (!std::isfinite(x0) || !std::isfinite(y0)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "x0 / y0 must be finite");
    if (!std::isfinite(dx) || !(dx > 0.0f)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "dx must be finite and > 0");
    if (!std::isfinite(dy) || !(dy > 0.0f)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "dy must be finite and > 0");
    if ((uint64_t)nx * ny >= (1ull << 31)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "nx * ny must be < 2^31");
    c->tsample.win[0] = c->tsample.win[1] = c->tsample.win[2] = c->tsample.win[3] = 0u;
    if ((uint64_t)nx * ny == 0) return SPHX_OK;
    if ((rc = tile_sample_state(c, fn))) return rc;
    const sphx_sample_host::Window w = sphx_sample_host::lattice_window(x0, y0, dx, dy, nx, ny, c->K.gmin_x, c->K.gmin_y, c->K.cell_inv, c->K.tile.x0,
                                                                      c->K.tile.x1, c->K.tile.y0, c->K.tile.y1);
    const size_t np = (size_t)w.points();
    if (!np) return SPHX_OK;  // no lattice point falls into a cell this tile owns
    SPHX_HIP(c, hipSetDevice(c->device));
    const size_t n_d = fields & SAMPLE_OUT_DENSITY ? np : 0, n_f = fields & SAMPLE_OUT_FRACTION ? np : 0, n_v = fields & SAMPLE_OUT_VELOCITY ? 2 * np : 0,
                 n_c = fields & SAMPLE_OUT_COUNT ? np : 0;
    if ((rc = tile_sample_scratch(c, n_d + n_f + n_v + n_c))) return rc;
    SampleArgs a{(const float2*)c->posA, (const float2*)c->vel, (const float*)c->density, c->soff(), NbGrid{}, NbGrid{}, nullptr, nullptr, nullptr, nullptr};
    if ((rc = tile_sample_grids(c, a.gd, a.gs))) return rc;
    float* p = c->sample_buf;
    a.o_density = n_d ? p : nullptr;
    p += n_d;
    a.o_fraction = n_f ? p : nullptr;
    p += n_f;
    a.o_velocity = n_v ? p : nullptr;
    p += n_v;
    a.o_count = n_c ? (uint32_t*)p : nullptr;
    hipStream_t st = c->stream;
    SPHX_HIP(c, hipMemsetAsync(c->sample_buf, 0, (n_d + n_f + n_v + n_c) * 4, st));  // (a lane that is not the owner writes nothing)
    const SampleLattice L{x0, y0, dx, dy, nx, ny, (nx + SAMPLE_TILE - 1) / SAMPLE_TILE};
    const SampleWindow W{w.ix0, w.iy0, w.w(), w.h(), (w.w() + SAMPLE_TILE - 1) / SAMPLE_TILE, w.w()};
    const uint32_t rev = c->K.rev;
    SampleJob q{nullptr, 0, &L, a};
    q.window = &W;
    enqueue_sample(c, q, kernel_kind, fields, np);
    c->K.rev = rev;
    c->tsample.win[0] = out_window[0] = w.ix0, c->tsample.win[1] = out_window[1] = w.ix1;
    c->tsample.win[2] = out_window[2] = w.iy0, c->tsample.win[3] = out_window[3] = w.iy1;
    c->tsample.fields = fields;
    return SPHX_OK;
}

int sphx_tile_sample_window_fetch(sphx_ctx* c, const sphx_sample_out* out) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_sample_window_fetch";
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out is NULL");
    if (!c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not a tile context");
    const uint32_t* const w = c->tsample.win;
    const size_t np = (size_t)(w[1] - w[0]) * (w[3] - w[2]);
    if (!np) return SPHX_OK;  // (an empty window, or none: nothing was queued)
    const uint32_t fields = c->tsample.fields;
    if (sample_outputs(out) != fields) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out does not name the fields of the queued query");
    c->tsample.win[0] = c->tsample.win[1] = c->tsample.win[2] = c->tsample.win[3] = 0u;
    SPHX_HIP(c, hipSetDevice(c->device));
    const float* p = c->sample_buf;
    hipStream_t st = c->stream;
    if (out->density) {
        SPHX_HIP(c, hipMemcpyAsync(out->density, p, np * 4, hipMemcpyDeviceToHost, st));
        p += np;
    }
    if (out->fraction) {
        SPHX_HIP(c, hipMemcpyAsync(out->fraction, p, np * 4, hipMemcpyDeviceToHost, st));
        p += np;
    }
    if (out->velocity) {
        SPHX_HIP(c, hipMemcpyAsync(out->velocity, p, 2 * np * 4, hipMemcpyDeviceToHost, st));
        p += 2 * np;
    }
    if (out->count) SPHX_HIP(c, hipMemcpyAsync(out->count, p, np * 4, hipMemcpyDeviceToHost, st));
    SPHX_HIP(c, hipStreamSynchronize(st));
    return SPHX_OK;
}

}  // extern "C"
