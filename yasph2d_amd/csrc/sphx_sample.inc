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
template <int KIND, bool DEN, bool FRAC, bool VEL>
__device__ __forceinline__ void sample_point(const Consts& K, const SampleArgs& a, float qx, float qy, bool live, uint32_t o) {
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
    if (!live) return;
    if (DEN && a.o_density) a.o_density[o] = rho;
    if (FRAC && a.o_fraction) a.o_fraction[o] = frac;
    if (VEL && a.o_velocity) {
        // Shepard-normalised; (0, 0) where no fluid particle contributes
        const bool some = frac != 0.0f;
        a.o_velocity[2 * (size_t)o] = some ? svx / frac : 0.0f;
        a.o_velocity[2 * (size_t)o + 1] = some ? svy / frac : 0.0f;
    }
    if (a.o_count) a.o_count[o] = cnt;
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
};

template <int KIND, bool DEN, bool FRAC, bool VEL>
void enqueue_sample_t(sphx_ctx* c, const SampleJob& q, uint64_t points) {
    // algorithmic bytes: the point (8, points path), the outputs, and ~ (9 cells) x (8-byte table entry) + the accepted records
    const double per = (q.lattice ? 0.0 : 8.0) + (DEN ? 4 : 0) + (FRAC ? 4 : 0) + (VEL ? 8 : 0) + 4 + 72.0;
    const uint32_t rev = c->K.rev;  // (a query must not change the sweep direction of the step's next kernels: launch() toggles it)
    hipStream_t st = c->stream;
    if (q.lattice) {
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
