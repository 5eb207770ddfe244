// sphx_stats.inc — fluid statistics (sphx_fluid_stats, sphx_stats_*, include/sphx.h): counts, float64 sums and exact extremes of the
// whole fluid and of up to eight probe rectangles, from ONE streaming pass over pos, vel and density (20 bytes per particle), instead
// of a sphx_download and a host loop.  Included at the end of sphx_kernels.hip (one translation unit: the launch layer of
// sphx_launch.inc is visible).  Everything here only READS the particle state (DESIGN.md §4i).
//
// Two launches, no atomics: stage 1 leaves one partial record per (workgroup, record) in a scratch array, stage 2 — one workgroup per
// record — folds them.  The grid and every order of addition are functions of N alone, so two calls on one state return the same bytes.

namespace sphx {

constexpr uint32_t STATS_TILE = 1024;      // particles per stage-1 workgroup the grid is sized by ...
constexpr uint32_t STATS_MAX_GRID = 2048;  // ... up to this many workgroups (8 per CU); beyond, the chunks grow
constexpr uint32_t STATS_MAX_REC = 1u + SPHX_STATS_MAX_RECTS;
static_assert(sizeof(sphx_stats_rec) == 128 && sizeof(sphx_stats_frame) == 16 && sizeof(sphx_stats_status) == 32, "the layouts of sphx.h");

struct StatsRects {
    sphx_rect r[SPHX_STATS_MAX_RECTS];
    uint32_t n;
};

inline uint32_t stats_grid(uint32_t n) { return std::min((n + STATS_TILE - 1u) / STATS_TILE, STATS_MAX_GRID); }
// a workgroup's contiguous chunk: a multiple of 256 (trailing workgroups may be left without particles: they write empty partials)
inline uint32_t stats_chunk(uint32_t n, uint32_t grid) { return grid ? ((n + grid - 1u) / grid + 255u) / 256u * 256u : 0u; }

// Extremes are kept as integer keys: key(f) is monotone in f over the finite floats and puts -0 below +0, so an integer min / max is
// exact, has no NaN or signed-zero cases and does not depend on the order of the operands.  key is its own inverse.
__device__ __forceinline__ int32_t stats_key(float f) {
    const int32_t i = __float_as_int(f);
    return i ^ ((i >> 31) & 0x7FFFFFFF);
}
__device__ __forceinline__ float stats_unkey(int32_t k) { return __int_as_float(k ^ ((k >> 31) & 0x7FFFFFFF)); }
constexpr int32_t STATS_KEY_PINF = 0x7F800000, STATS_KEY_NINF = (int32_t)0x807FFFFFu;  // key(+inf), key(-inf)

// the running state of one record: what a lane, a wavefront, a workgroup or the whole grid has seen so far
struct StatsAcc {
    double s[8];  // sum_pos x, y; sum_vel x, y; sum_speed_sq; sum_angular; sum_density; sum_density_sq
    double vmax;  // max_speed_sq
    int32_t mn[3], mx[3];  // keys of x, y, density
    unsigned long long cnt[3];  // count, nonfinite, density_count
};
__device__ __forceinline__ void stats_clear(StatsAcc& a) {
#pragma unroll
    for (int j = 0; j < 8; ++j) a.s[j] = 0.0;
    a.vmax = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) a.mn[j] = STATS_KEY_PINF, a.mx[j] = STATS_KEY_NINF, a.cnt[j] = 0ull;
}
// a = a (+) b without the counts: every sum is a + b in this order
__device__ __forceinline__ void stats_merge_values(StatsAcc& a, const StatsAcc& b) {
#pragma unroll
    for (int j = 0; j < 8; ++j) a.s[j] = a.s[j] + b.s[j];
    a.vmax = fmax(a.vmax, b.vmax);
#pragma unroll
    for (int j = 0; j < 3; ++j) a.mn[j] = min(a.mn[j], b.mn[j]), a.mx[j] = max(a.mx[j], b.mx[j]);
}
__device__ __forceinline__ void stats_merge(StatsAcc& a, const StatsAcc& b) {
    stats_merge_values(a, b);
#pragma unroll
    for (int j = 0; j < 3; ++j) a.cnt[j] += b.cnt[j];
}
// The value of another lane of the same row of 16 by a DPP move (no LDS traffic): 0xB1 / 0x4E = quad_perm [1,0,3,2] / [2,3,0,1] (lane ^ 1,
// lane ^ 2), 0x141 = row_half_mirror (7 - lane within 8), 0x140 = row_mirror (15 - lane within 16).  Every lane has a source.
template <int CTRL>
__device__ __forceinline__ int32_t stats_dpp(int32_t v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ double stats_dpp(double v) {
    return __hiloint2double(stats_dpp<CTRL>(__double2hiint(v)), stats_dpp<CTRL>(__double2loint(v)));
}
template <int CTRL>
__device__ __forceinline__ void stats_row_step(StatsAcc& a) {
#pragma unroll
    for (int j = 0; j < 8; ++j) a.s[j] = a.s[j] + stats_dpp<CTRL>(a.s[j]);
    a.vmax = fmax(a.vmax, stats_dpp<CTRL>(a.vmax));
#pragma unroll
    for (int j = 0; j < 3; ++j) a.mn[j] = min(a.mn[j], stats_dpp<CTRL>(a.mn[j])), a.mx[j] = max(a.mx[j], stats_dpp<CTRL>(a.mx[j]));
}
// all-reduce over the 64 lanes in a fixed order: pairs, quads, eights and the row of 16 by DPP, then the four rows by two shuffles
// (IEEE addition is commutative: both partners of a step form the same bits, so every lane ends with the same value)
__device__ __forceinline__ void stats_wave_values(StatsAcc& a) {
    stats_row_step<0xB1>(a);
    stats_row_step<0x4E>(a);
    stats_row_step<0x141>(a);
    stats_row_step<0x140>(a);
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) a.s[j] = a.s[j] + __shfl_xor(a.s[j], off);
        a.vmax = fmax(a.vmax, __shfl_xor(a.vmax, off));
#pragma unroll
        for (int j = 0; j < 3; ++j) a.mn[j] = min(a.mn[j], __shfl_xor(a.mn[j], off)), a.mx[j] = max(a.mx[j], __shfl_xor(a.mx[j], off));
    }
}
__device__ __forceinline__ void stats_wave_counts(StatsAcc& a) {
#pragma unroll
    for (int off = 32; off; off >>= 1)
#pragma unroll
        for (int j = 0; j < 3; ++j) a.cnt[j] += __shfl_xor(a.cnt[j], off);
}
__device__ __forceinline__ void stats_to_rec(const StatsAcc& a, uint32_t density_valid, sphx_stats_rec& r) {
    r.count = a.cnt[0], r.nonfinite = a.cnt[1], r.density_count = a.cnt[2];
    r.density_valid = density_valid, r.reserved = 0u;
    r.sum_pos[0] = a.s[0], r.sum_pos[1] = a.s[1], r.sum_vel[0] = a.s[2], r.sum_vel[1] = a.s[3];
    r.sum_speed_sq = a.s[4], r.sum_angular = a.s[5], r.sum_density = a.s[6], r.sum_density_sq = a.s[7];
    r.max_speed_sq = a.vmax;
    r.min_pos[0] = stats_unkey(a.mn[0]), r.min_pos[1] = stats_unkey(a.mn[1]), r.max_pos[0] = stats_unkey(a.mx[0]), r.max_pos[1] = stats_unkey(a.mx[1]);
    r.min_density = stats_unkey(a.mn[2]), r.max_density = stats_unkey(a.mx[2]);
}
__device__ __forceinline__ void stats_from_rec(const sphx_stats_rec& r, StatsAcc& a) {
    a.cnt[0] = r.count, a.cnt[1] = r.nonfinite, a.cnt[2] = r.density_count;
    a.s[0] = r.sum_pos[0], a.s[1] = r.sum_pos[1], a.s[2] = r.sum_vel[0], a.s[3] = r.sum_vel[1];
    a.s[4] = r.sum_speed_sq, a.s[5] = r.sum_angular, a.s[6] = r.sum_density, a.s[7] = r.sum_density_sq;
    a.vmax = r.max_speed_sq;
    a.mn[0] = stats_key(r.min_pos[0]), a.mn[1] = stats_key(r.min_pos[1]), a.mx[0] = stats_key(r.max_pos[0]), a.mx[1] = stats_key(r.max_pos[1]);
    a.mn[2] = stats_key(r.min_density), a.mx[2] = stats_key(r.max_density);
}

// Stage 1.  Workgroup b owns the particles [b * chunk, min(n, (b + 1) * chunk)) and walks them 256 at a time, one particle per lane,
// the next trip's loads issued before this trip's arithmetic.  Record 0 is summed per lane over the trips, then over the lanes, then
// over the four wavefronts.  A rectangle is decided per wavefront: the particles are cell-sorted, so most wavefronts lie outside most
// rectangles and a ballot skips them; a wavefront with a lane inside reduces that trip's masked terms at once and its lane 0 adds them
// to the wavefront's accumulator of that rectangle in LDS — no lane carries a set of sums per rectangle.  `density` is null while
// density[] does not belong to the positions: nothing of it is read.  The partial records go out with plain stores.
// OWNED (a tile context: sphx_tile_fluid_stats) also streams pid[]: only a particle the tile owns — bit 31 of its id — is live; a ghost
// enters no count, no sum, no extreme and no rectangle (24 bytes per particle instead of 20).  NT: pid[] by nontemporal loads, the
// policy of k_track_lookup.  Without OWNED pid is not read and the kernel is the single context's, instruction for instruction.
template <bool OWNED, bool NT = false>
__global__ __launch_bounds__(256) void k_stats_partial(const float2* __restrict__ pos, const float2* __restrict__ vel, const float* __restrict__ density,
                                                       uint32_t n, uint32_t chunk, StatsRects R, sphx_stats_rec* __restrict__ partial,
                                                       const uint32_t* __restrict__ pid) {
    __shared__ StatsAcc wacc[4][STATS_MAX_REC];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t nrec = 1u + R.n;
    if (lane < nrec) stats_clear(wacc[wave][lane]);
    __syncthreads();
    const uint32_t begin = blockIdx.x * chunk;  // (grid * chunk < n + 256 * grid: no overflow for n < 2^28)
    const uint32_t end = begin < n ? min(n, begin + chunk) : begin;
    StatsAcc a;
    stats_clear(a);
    uint32_t i = begin + threadIdx.x;
    float2 p = make_float2(0.0f, 0.0f), v = p;
    float rho = 0.0f;
    uint32_t id = 0u;  // (OWNED only)
    if (i < end) {
        p = pos[i], v = vel[i];
        if (density) rho = density[i];
        if constexpr (OWNED) id = NT ? __builtin_nontemporal_load(pid + i) : pid[i];
    }
    for (uint32_t base = begin; base < end; base += 256u, i += 256u) {
        bool live = i < end;
        if constexpr (OWNED) live = live && (id >> 31);
        const float2 pc = p, vc = v;
        const float rc = rho;
        if (i + 256u < end) {
            p = pos[i + 256u], v = vel[i + 256u];
            if (density) rho = density[i + 256u];
            if constexpr (OWNED) id = NT ? __builtin_nontemporal_load(pid + i + 256u) : pid[i + 256u];
        }
        const bool fin = live && isfinite(pc.x) && isfinite(pc.y) && isfinite(vc.x) && isfinite(vc.y);
        const bool dfin = fin && density != nullptr && isfinite(rc);
        const double x = (double)pc.x, y = (double)pc.y, vx = (double)vc.x, vy = (double)vc.y, d = (double)rc;
        const double t_speed = vx * vx + vy * vy, t_ang = x * vy - y * vx, t_dsq = d * d;  // (exact products: one rounding per term)
        const int32_t kx = stats_key(pc.x), ky = stats_key(pc.y), kd = stats_key(rc);
        if (fin) {
            a.s[0] = a.s[0] + x, a.s[1] = a.s[1] + y, a.s[2] = a.s[2] + vx, a.s[3] = a.s[3] + vy;
            a.s[4] = a.s[4] + t_speed, a.s[5] = a.s[5] + t_ang;
            a.vmax = fmax(a.vmax, t_speed);
            a.mn[0] = min(a.mn[0], kx), a.mx[0] = max(a.mx[0], kx), a.mn[1] = min(a.mn[1], ky), a.mx[1] = max(a.mx[1], ky);
            a.cnt[0] += 1ull;
        }
        if (live && !fin) a.cnt[1] += 1ull;
        if (dfin) {
            a.s[6] = a.s[6] + d, a.s[7] = a.s[7] + t_dsq;
            a.mn[2] = min(a.mn[2], kd), a.mx[2] = max(a.mx[2], kd);
            a.cnt[2] += 1ull;
        }
        for (uint32_t k = 0; k < R.n; ++k) {
            const sphx_rect r = R.r[k];
            const bool in = live && pc.x >= r.x0 && pc.x < r.x1 && pc.y >= r.y0 && pc.y < r.y1;  // (sphx_remove's predicate: a NaN is in no rectangle)
            const unsigned long long b_in = __ballot(in);
            if (!b_in) continue;  // (wavefront-uniform)
            const unsigned long long b_fin = __ballot(in && fin), b_dfin = __ballot(in && dfin);
            StatsAcc m;
            stats_clear(m);
            if (in && fin) {
                m.s[0] = x, m.s[1] = y, m.s[2] = vx, m.s[3] = vy, m.s[4] = t_speed, m.s[5] = t_ang;
                m.vmax = t_speed;
                m.mn[0] = m.mx[0] = kx, m.mn[1] = m.mx[1] = ky;
            }
            if (in && dfin) {
                m.s[6] = d, m.s[7] = t_dsq;
                m.mn[2] = m.mx[2] = kd;
            }
            if (b_fin) stats_wave_values(m);  // (no finite lane inside: only the non-finite count moves)
            if (lane == 0u) {
                StatsAcc w = wacc[wave][1u + k];
                stats_merge_values(w, m);
                w.cnt[0] += (unsigned long long)__popcll(b_fin);
                w.cnt[1] += (unsigned long long)__popcll(b_in & ~b_fin);
                w.cnt[2] += (unsigned long long)__popcll(b_dfin);
                wacc[wave][1u + k] = w;
            }
        }
    }
    stats_wave_values(a);
    stats_wave_counts(a);
    if (lane == 0u) wacc[wave][0] = a;
    __syncthreads();
    if (threadIdx.x < nrec) {
        StatsAcc f = wacc[0][threadIdx.x];
        stats_merge(f, wacc[1][threadIdx.x]);
        stats_merge(f, wacc[2][threadIdx.x]);
        stats_merge(f, wacc[3][threadIdx.x]);
        sphx_stats_rec out;
        stats_to_rec(f, 0u, out);
        partial[(size_t)blockIdx.x * nrec + threadIdx.x] = out;
    }
}

// Stage 2: workgroup r folds the `grid` partial records of record r — lane l takes the partials l, l + 256, ... in ascending order,
// then the lanes, then the four wavefronts — and writes the record (grid == 0: the empty record).
__global__ __launch_bounds__(256) void k_stats_combine(const sphx_stats_rec* __restrict__ partial, uint32_t grid, uint32_t nrec, uint32_t density_valid,
                                                       sphx_stats_rec* __restrict__ out) {
    __shared__ StatsAcc wacc[4];
    const uint32_t r = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    StatsAcc a;
    stats_clear(a);
    for (uint32_t g = threadIdx.x; g < grid; g += 256u) {
        StatsAcc b;
        stats_from_rec(partial[(size_t)g * nrec + r], b);
        stats_merge(a, b);
    }
    stats_wave_values(a);
    stats_wave_counts(a);
    if (lane == 0u) wacc[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0u) {
        StatsAcc f = wacc[0];
        stats_merge(f, wacc[1]);
        stats_merge(f, wacc[2]);
        stats_merge(f, wacc[3]);
        sphx_stats_rec o;
        stats_to_rec(f, density_valid, o);
        out[r] = o;
    }
}

}  // namespace sphx

// ---- launch layer and C ABI ----------------------------------------------------------------------------------------------------------
namespace {

constexpr size_t STATS_PARTIALS = (size_t)STATS_MAX_GRID * STATS_MAX_REC;  // records of the stage-1 scratch
constexpr uint64_t STATS_REC_BYTES_MAX = 64ull << 20;                      // a recording's device buffer

// NULL rects with n_rects > 0, too many rectangles, a NaN bound -> the message; nullptr: fine
const char* stats_check_rects(const sphx_rect* rects, uint32_t n_rects) {
    if (n_rects > SPHX_STATS_MAX_RECTS) return "n_rects exceeds SPHX_STATS_MAX_RECTS";
    if (n_rects && !rects) return "rects is NULL with n_rects > 0";
    for (uint32_t k = 0; k < n_rects; ++k)
        if (std::isnan(rects[k].x0) || std::isnan(rects[k].y0) || std::isnan(rects[k].x1) || std::isnan(rects[k].y1)) return "rects holds a NaN bound";
    return nullptr;
}
int stats_check_ctx(sphx_ctx* c, const char* fn) {
    const std::string f = fn;
    if (c->tile_mode)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": not available on a tile context (its arrays hold ghosts and miss the particles other tiles own)").c_str());
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, (f + ": between step_begin and step_finish (finish the step first)").c_str());
    return SPHX_OK;
}

// the stage-1 partials and, behind them, the records of one host-pointer call; allocated once
int stats_scratch(sphx_ctx* c) {
    if (c->stats.scratch) return SPHX_OK;
    return dev_alloc(c, &c->stats.scratch, STATS_PARTIALS + STATS_MAX_REC);
}

// both stages behind what is on the stream, 1 + n_rects records to `out` (device); the sweep direction launch() toggles is put back.
// owned (a tile context): the records cover the particles the tile owns.  n is the local count the host holds since the tile's last
// re-grid (sphx_sub_regrid leaves the exact one in c->N, like for every other kernel of the tile path): nothing is waited for.
void stats_enqueue(sphx_ctx* c, const sphx_rect* rects, uint32_t n_rects, sphx_stats_rec* out, bool owned = false) {
    sphx_ctx::Stats& s = c->stats;
    const uint32_t n = c->N, nrec = 1u + n_rects;
    // a tile's densities are those of its last re-grid (sub_regrid_impl: every re-grid of the tile path computes them with the lists)
    const uint32_t density_valid = owned ? (c->tile_density_ready ? 1u : 0u) : (c->uploaded && c->sample_ready == 2u ? 1u : 0u);
    const uint32_t grid = stats_grid(n), chunk = stats_chunk(n, grid);
    StatsRects R{};
    for (uint32_t k = 0; k < n_rects; ++k) R.r[k] = rects[k];
    R.n = n_rects;
    const uint32_t rev = c->K.rev;
    hipStream_t st = c->stream;
    if (grid && owned)
        launch(c, "stats_partial", (density_valid ? 24.0 : 20.0) * n, [&] {
            if (n >= TRACK_NT_FROM)
                hipLaunchKernelGGL((k_stats_partial<true, true>), dim3(grid), dim3(256), 0, st, (const float2*)c->posA, (const float2*)c->vel,
                                   density_valid ? (const float*)c->density : (const float*)nullptr, n, chunk, R, s.scratch, (const uint32_t*)c->pid);
            else
                hipLaunchKernelGGL((k_stats_partial<true, false>), dim3(grid), dim3(256), 0, st, (const float2*)c->posA, (const float2*)c->vel,
                                   density_valid ? (const float*)c->density : (const float*)nullptr, n, chunk, R, s.scratch, (const uint32_t*)c->pid);
        });
    else if (grid)
        launch(c, "stats_partial", (density_valid ? 20.0 : 16.0) * n, [&] {
            hipLaunchKernelGGL((k_stats_partial<false>), dim3(grid), dim3(256), 0, st, (const float2*)c->posA, (const float2*)c->vel,
                               density_valid ? (const float*)c->density : (const float*)nullptr, n, chunk, R, s.scratch, (const uint32_t*)nullptr);
        });
    launch(c, "stats_combine", 128.0 * nrec * (grid + 1.0), [&] {
        hipLaunchKernelGGL(k_stats_combine, dim3(nrec), dim3(256), 0, st, (const sphx_stats_rec*)s.scratch, grid, nrec, density_valid, out);
    });
    c->K.rev = rev;
}

void stats_drop_recording(sphx_ctx* c) {
    sphx_ctx::Stats& s = c->stats;
    dev_free(&s.rec);
    s.info.clear();
    s.info.shrink_to_fit();
    s.n_rects = s.recording = s.max_frames = s.every = s.frames = s.dropped = s.steps = 0;
}

// One frame behind the kernels of the step that has just finished (sphx_step_finish / sphx_wcsph_step_finish call this through
// stats_after_step when a recording is on).  Nothing comes back to the host.
void stats_take_frame(sphx_ctx* c, float dt) {
    sphx_ctx::Stats& s = c->stats;
    if (c->tile_mode) return;
    if (++s.steps % s.every) return;
    if (s.frames >= s.max_frames) {
        s.dropped += 1u;
        return;
    }
    stats_enqueue(c, s.rects, s.n_rects, s.rec + (size_t)s.frames * (1u + s.n_rects));
    s.info.push_back(sphx_stats_frame{s.steps, dt, c->N});
    s.frames += 1u;
}

}  // namespace

extern "C" {

int sphx_fluid_stats(sphx_ctx* c, const sphx_rect* rects, uint32_t n_rects, uint32_t flags, sphx_stats_rec* out) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_fluid_stats: out is NULL");
    if (const char* bad = stats_check_rects(rects, n_rects)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_fluid_stats", bad);
    if (flags & ~(uint32_t)SPHX_STATS_DEVICE_POINTERS) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_fluid_stats: unknown flags bits");
    const bool dev = flags & SPHX_STATS_DEVICE_POINTERS;
    if (dev && ((uintptr_t)out & 7u)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_fluid_stats: out (a device pointer) is not 8-byte aligned");
    int rc;
    if ((rc = stats_check_ctx(c, "sphx_fluid_stats"))) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    flush_pending_advect(c);
    if ((rc = stats_scratch(c))) return rc;
    if (dev) {
        stats_enqueue(c, rects, n_rects, out);
        return SPHX_OK;
    }
    sphx_stats_rec* const d_out = c->stats.scratch + STATS_PARTIALS;
    stats_enqueue(c, rects, n_rects, d_out);
    SPHX_HIP(c, hipMemcpyAsync(out, d_out, (size_t)(1u + n_rects) * sizeof(sphx_stats_rec), hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    return SPHX_OK;
}

int sphx_stats_record(sphx_ctx* c, const sphx_rect* rects, uint32_t n_rects, uint32_t max_frames, uint32_t every) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = stats_check_ctx(c, "sphx_stats_record"))) return rc;
    if (max_frames) {  // (max_frames == 0 stops and frees, whatever the other arguments say)
        if (const char* bad = stats_check_rects(rects, n_rects)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_stats_record", bad);
        if (every == 0) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_stats_record: every must be >= 1");
        if ((uint64_t)max_frames * (1u + n_rects) * sizeof(sphx_stats_rec) > STATS_REC_BYTES_MAX)
            return c->fail(SPHX_ERR_CAPACITY, "sphx_stats_record: max_frames * (1 + n_rects) records exceed 64 MiB");
    }
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));  // (a queued frame may still write the old buffer)
    stats_drop_recording(c);
    if (!max_frames) return SPHX_OK;
    if ((rc = stats_scratch(c))) return rc;
    sphx_ctx::Stats& s = c->stats;
    if ((rc = dev_alloc(c, &s.rec, (size_t)max_frames * (1u + n_rects)))) return rc;
    for (uint32_t k = 0; k < n_rects; ++k) s.rects[k] = rects[k];
    s.n_rects = n_rects;
    s.max_frames = max_frames;
    s.every = every;
    s.recording = 1u;
    return SPHX_OK;
}

int sphx_stats_get_status(const sphx_ctx* c, sphx_stats_status* out) {
    if (!c || !out) return SPHX_ERR_INVALID_ARGUMENT;
    const sphx_ctx::Stats& s = c->stats;
    std::memset(out, 0, sizeof(*out));
    out->n_rects = s.n_rects;
    out->recording = s.recording;
    out->max_frames = s.max_frames;
    out->every = s.every;
    out->frames = s.frames;
    out->dropped = s.dropped;
    return SPHX_OK;
}

int sphx_stats_read(sphx_ctx* c, uint32_t first_frame, uint32_t n_frames, sphx_stats_rec* out, sphx_stats_frame* info) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = stats_check_ctx(c, "sphx_stats_read"))) return rc;
    const sphx_ctx::Stats& s = c->stats;
    if ((uint64_t)first_frame + n_frames > s.frames)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_stats_read: first_frame + n_frames is beyond the frames recorded (sphx_stats_get_status)");
    if (n_frames == 0) return SPHX_OK;
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_stats_read: out is NULL");
    SPHX_HIP(c, hipSetDevice(c->device));
    const size_t frame = 1u + s.n_rects;  // records
    SPHX_HIP(c, hipMemcpyAsync(out, s.rec + first_frame * frame, n_frames * frame * sizeof(sphx_stats_rec), hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    if (info) std::memcpy(info, s.info.data() + first_frame, (size_t)n_frames * sizeof(sphx_stats_frame));
    return SPHX_OK;
}

// ---- one tile of a tiled run (sphx_multi_fluid_stats and the multi recorder, sphx_tiles.cpp, are built on these) ------------------------
namespace {
int stats_check_tile(sphx_ctx* c, const char* fn) {
    const std::string f = fn;
    if (!c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": not a tile context (sphx_fluid_stats and sphx_stats_* serve a plain one)").c_str());
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, (f + ": between step_begin and step_finish (finish the step first)").c_str());
    return SPHX_OK;
}
// between the packing pass and the re-grid the local count is an upper bound and an advection may be pending: no statistics of that
int stats_check_tile_state(sphx_ctx* c, const char* fn) {
    if (c->N && (!c->lists_current || c->tile_pending_dt > 0.0f))
        return c->fail(SPHX_ERR_NOT_READY, (std::string(fn) + ": the tile is between a halo exchange and its re-grid (sphx_sub_regrid first)").c_str());
    return SPHX_OK;
}
}  // namespace

int sphx_tile_fluid_stats(sphx_ctx* c, const sphx_rect* rects, uint32_t n_rects, uint32_t flags, sphx_stats_rec* out) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_fluid_stats: out is NULL");
    if (const char* bad = stats_check_rects(rects, n_rects)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_fluid_stats", bad);
    if (flags & ~(uint32_t)SPHX_STATS_DEVICE_POINTERS) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_fluid_stats: unknown flags bits");
    const bool dev = flags & SPHX_STATS_DEVICE_POINTERS;
    if (dev && ((uintptr_t)out & 7u)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_fluid_stats: out (a device pointer) is not 8-byte aligned");
    int rc;
    if ((rc = stats_check_tile(c, "sphx_tile_fluid_stats"))) return rc;
    if ((rc = stats_check_tile_state(c, "sphx_tile_fluid_stats"))) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    if ((rc = stats_scratch(c))) return rc;
    if (dev) {
        stats_enqueue(c, rects, n_rects, out, true);
        return SPHX_OK;
    }
    sphx_stats_rec* const d_out = c->stats.scratch + STATS_PARTIALS;
    stats_enqueue(c, rects, n_rects, d_out, true);
    SPHX_HIP(c, hipMemcpyAsync(out, d_out, (size_t)(1u + n_rects) * sizeof(sphx_stats_rec), hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    return SPHX_OK;
}

int sphx_tile_stats_record(sphx_ctx* c, const sphx_rect* rects, uint32_t n_rects, uint32_t max_frames, uint32_t every) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = stats_check_tile(c, "sphx_tile_stats_record"))) return rc;
    if (max_frames) {  // (max_frames == 0 stops and frees, whatever the other arguments say)
        if (const char* bad = stats_check_rects(rects, n_rects)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_stats_record", bad);
        if (every == 0) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_stats_record: every must be >= 1");
        if ((uint64_t)max_frames * (1u + n_rects) * sizeof(sphx_stats_rec) > STATS_REC_BYTES_MAX)
            return c->fail(SPHX_ERR_CAPACITY, "sphx_tile_stats_record: max_frames * (1 + n_rects) records exceed 64 MiB");
    }
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));  // (a queued frame may still write the old buffer)
    stats_drop_recording(c);
    if (!max_frames) return SPHX_OK;
    if ((rc = stats_scratch(c))) return rc;
    sphx_ctx::Stats& s = c->stats;
    if ((rc = dev_alloc(c, &s.rec, (size_t)max_frames * (1u + n_rects)))) return rc;
    for (uint32_t k = 0; k < n_rects; ++k) s.rects[k] = rects[k];
    s.n_rects = n_rects;
    s.max_frames = max_frames;
    s.every = every;
    s.recording = 1u;
    return SPHX_OK;
}

// The tile loop calls this at the end of every finished step: with a recording on, every `every`-th call queues one frame of the owned
// particles behind the step's kernels.  n_global is the owned count of the whole run (the tile loop has it from its last all-reduce).
// Nothing comes back to the host and nothing is waited for.
int sphx_tile_stats_frame(sphx_ctx* c, float dt, uint32_t n_global) {
    if (!c || !c->tile_mode) return SPHX_ERR_INVALID_ARGUMENT;
    sphx_ctx::Stats& s = c->stats;
    if (!s.recording) return SPHX_OK;
    if (++s.steps % s.every) return SPHX_OK;
    if (s.frames >= s.max_frames) {
        s.dropped += 1u;
        return SPHX_OK;
    }
    int rc;
    if ((rc = stats_check_tile_state(c, "sphx_tile_stats_frame"))) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    stats_enqueue(c, s.rects, s.n_rects, s.rec + (size_t)s.frames * (1u + s.n_rects), true);
    s.info.push_back(sphx_stats_frame{s.steps, dt, n_global});
    s.frames += 1u;
    return SPHX_OK;
}

int sphx_tile_stats_read(sphx_ctx* c, uint32_t first_frame, uint32_t n_frames, sphx_stats_rec* out, sphx_stats_frame* info) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = stats_check_tile(c, "sphx_tile_stats_read"))) return rc;
    const sphx_ctx::Stats& s = c->stats;
    if ((uint64_t)first_frame + n_frames > s.frames)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_stats_read: first_frame + n_frames is beyond the frames recorded (sphx_stats_get_status)");
    if (n_frames == 0) return SPHX_OK;
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_stats_read: out is NULL");
    SPHX_HIP(c, hipSetDevice(c->device));
    const size_t frame = 1u + s.n_rects;  // records
    SPHX_HIP(c, hipMemcpyAsync(out, s.rec + first_frame * frame, n_frames * frame * sizeof(sphx_stats_rec), hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    if (info) std::memcpy(info, s.info.data() + first_frame, (size_t)n_frames * sizeof(sphx_stats_frame));
    return SPHX_OK;
}

}  // extern "C"
