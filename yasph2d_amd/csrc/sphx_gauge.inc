// sphx_gauge.inc — water levels along rays (sphx_gauge_levels, sphx_gauge_reduce) and the per-step recorder of gauge records and point
// probes (sphx_probe_*); the contract is in include/sphx.h, "gauges and probes", restated bit for bit by tests/gauge_reference.py.
// Included in sphx_kernels.hip behind sphx_sample.inc (one translation unit, -ffp-contract=off): the values are sample_walk's, the
// record is sphx_gauge_rule.hpp's, on the host and on the device alike.  Two passes, whatever the number of gauges:
//   k_gauge_sample  the samples of all gauges laid flat, 256 per workgroup, a lane per sample: one 4-byte value each;
//   k_gauge_reduce  a wavefront per gauge walks its values in trips of 64: ballots of the inside test give first / last / inside, two
//                   values are read back and lane 0 stores the record.  No LDS, no atomic, plain loads and stores.
// A recorded frame adds k_probe_points: sample_walk at the fixed points, a 32-byte sphx_probe_rec per point.
// A tile of a tiled run (sphx_tile_gauge_* / sphx_tile_probe_*, the seam of sphx_multi_gauge_levels and sphx_multi_probe_*) runs the
// k_tile_* twins over the samples it owns and stores a 32-byte sphx_gauge_part per gauge; the host folds the parts (sphx_gauge_merge.hpp).

#include "sphx_gauge_rule.hpp"
#include "sphx_gauge_merge.hpp"

namespace sphx {

// The gauge table on the device: the caller's sphx_gauge with reserved[0] = the flat index of its first sample (an exclusive prefix of n).
constexpr uint32_t GAUGE_OFF = 0;  // index into sphx_gauge::reserved

// The table reaches the device as kernel arguments, 64 gauges (2 KiB) per launch: nothing is copied from host memory that the call
// would have to wait for, so the device-pointer path is enqueued and returns.
constexpr uint32_t GAUGE_CHUNK = 64;
struct GaugeChunk {
    sphx_gauge g[GAUGE_CHUNK];
};
__global__ __launch_bounds__(64) void k_gauge_table(GaugeChunk ch, uint32_t count, sphx_gauge* __restrict__ tab) {
    if (threadIdx.x < count) tab[threadIdx.x] = ch.g[threadIdx.x];
}

// sample pass: flat sample blockIdx.x * 256 + threadIdx.x (total <= 2^24: one launch).  Consecutive lanes are consecutive samples of one
// ray but where a gauge ends inside the wavefront: their 3 x 3 boxes overlap, as on the lattice path.  A dead lane (behind the last
// sample) makes the walk's call with live = false, like every caller of sample_walk.
template <int KIND, bool DEN>
__global__ __launch_bounds__(256) void k_gauge_sample(Consts K, SampleArgs a, const sphx_gauge* __restrict__ tab, uint32_t n_gauges, uint32_t total,
                                                      float* __restrict__ values) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool live = i < total;
    const uint32_t j = live ? i : total - 1u;  // (total > 0: the host launches nothing for an empty set)
    // the gauge of sample j: the last one whose first sample is <= j (tab[0] starts at 0)
    uint32_t lo = 0, hi = n_gauges;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab[mid].reserved[GAUGE_OFF] <= j) lo = mid;
        else hi = mid;
    }
    const sphx_gauge g = tab[lo];
    const uint32_t k = j - g.reserved[GAUGE_OFF];
    const float qx = g.x0 + (float)k * g.dx;
    const float qy = g.y0 + (float)k * g.dy;
    const SampleSums r = sample_walk<KIND, DEN, !DEN, false>(K, a, qx, qy, live);
    if (live) values[j] = DEN ? r.rho : r.frac;
}

// reduction pass: wavefront w of workgroup b owns gauge 4 b + w.  The loop bounds are the gauge's: all 64 lanes are active at the ballot.
__global__ __launch_bounds__(256) void k_gauge_reduce(const sphx_gauge* __restrict__ tab, uint32_t n_gauges, const float* __restrict__ values, float iso,
                                                      uint32_t* __restrict__ out) {
    const uint32_t gi = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (gi >= n_gauges) return;  // (wavefront-uniform)
    const sphx_gauge g = tab[gi];
    const float* const f = values + g.reserved[GAUGE_OFF];
    uint32_t first = SPHX_GAUGE_NONE, last = SPHX_GAUGE_NONE, inside = 0;
    for (uint32_t k0 = 0; k0 < g.n; k0 += 64u) {
        const uint32_t k = k0 + lane;
        const bool b = k < g.n && f[k] >= iso;  // (a lane behind the ray loads nothing; NaN: outside)
        const unsigned long long m = __ballot(b);
        if (m) {
            if (!inside) first = k0 + (uint32_t)__ffsll((long long)m) - 1u;
            last = k0 + 63u - (uint32_t)__clzll((long long)m);
            inside += (uint32_t)__popcll(m);
        }
    }
    if (lane != 0u) return;
    const float f_last = inside ? f[last] : 0.0f;
    const float f_next = inside && last + 1u < g.n ? f[last + 1u] : 0.0f;
    const sphx_gauge_host::Words r = sphx_gauge_host::record(g, iso, first, last, inside, f_last, f_next);
    uint32_t* const o = out + 8 * (size_t)gi;  // (4-byte aligned is all the contract asks of a device `out`)
#pragma unroll
    for (int w = 0; w < 8; ++w) o[w] = r.w[w];
}

// point probes of a frame: sphx_sample_points' four outputs at point blockIdx.x * 256 + threadIdx.x, as one sphx_probe_rec (two 16-byte
// stores; the frames start on 32-byte multiples of a hipMalloc'ed buffer)
template <int KIND>
__global__ __launch_bounds__(256) void k_probe_points(Consts K, SampleArgs a, const float* __restrict__ xy, uint32_t m, uint4* __restrict__ rec) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool live = i < m;
    const uint32_t k = live ? i : m - 1u;  // (m > 0)
    const SampleSums r = sample_walk<KIND, true, true, true>(K, a, xy[2 * (size_t)k], xy[2 * (size_t)k + 1], live);
    if (!live) return;
    const float2 v = sample_velocity(r);
    rec[2 * (size_t)k] = make_uint4(__float_as_uint(r.rho), __float_as_uint(r.frac), __float_as_uint(v.x), __float_as_uint(v.y));
    rec[2 * (size_t)k + 1] = make_uint4(r.cnt, 0u, 0u, 0u);
}

// ---- one tile of a tiled run (sphx_tile_gauge_* / sphx_tile_probe_*, include/sphx.h "gauges and probes of a tiled run") ------------------
// A tile answers the samples whose cell lies in its owned rectangle K.tile.  On one gauge they are ONE contiguous index interval
// (sphx_gauge_window.hpp, fact 1), which the host finds by bisection: the tile's table holds, per gauge, the caller's ray with
// reserved[GAUGE_OFF] = the compact index of the interval's first value (an exclusive prefix of the counts), reserved[GAUGE_LO] = lo and
// reserved[GAUGE_CNT] = count.  The K tiles of a run together walk the samples of one call.  Both passes test the ownership again with
// the device's own expression: the part reports the count the DEVICE accepted, and the fold refuses parts that do not tile the ray.
constexpr uint32_t GAUGE_LO = 1, GAUGE_CNT = 2;  // indices into sphx_gauge::reserved

// sample pass: compact sample blockIdx.x * 256 + threadIdx.x of the tile's `total` owned samples (total > 0).  A lane whose sample the
// tile does not own after all walks nothing and stores the word 0x7FC00000.
template <int KIND, bool DEN>
__global__ __launch_bounds__(256) void k_tile_gauge_sample(Consts K, SampleArgs a, const sphx_gauge* __restrict__ tab, uint32_t n_gauges, uint32_t total,
                                                           float* __restrict__ values) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool live = i < total;
    const uint32_t j = live ? i : total - 1u;
    // the gauge of compact sample j: the last one whose first value is <= j (a gauge without owned samples shares its successor's index
    // and is never the last such)
    uint32_t lo = 0, hi = n_gauges;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab[mid].reserved[GAUGE_OFF] <= j) lo = mid;
        else hi = mid;
    }
    const sphx_gauge g = tab[lo];
    const uint32_t k = g.reserved[GAUGE_LO] + (j - g.reserved[GAUGE_OFF]);  // the GLOBAL sample index: the point is the single context's
    const float qx = g.x0 + (float)k * g.dx;
    const float qy = g.y0 + (float)k * g.dy;
    uint32_t cx, cy;
    cell_of(K, make_float2(qx, qy), cx, cy);
    const bool own = rect_has(K.tile, cx, cy, 0u);
    const SampleSums r = sample_walk<KIND, DEN, !DEN, false>(K, a, qx, qy, live && own);
    if (live) values[j] = own ? (DEN ? r.rho : r.frac) : __uint_as_float(sphx_gauge_host::QNAN_WORD);
}

// reduce pass: wavefront w of workgroup b owns gauge 4 b + w and walks the tile's interval of it in trips of 64.  Ballots of the
// ownership test give the count, ballots of the inside test first / last / inside; three values are read back and lane 0 stores the
// sphx_gauge_part.  The loop bounds are the gauge's: all 64 lanes are active at the ballots.  No LDS, no atomic.
__global__ __launch_bounds__(256) void k_tile_gauge_reduce(Consts K, const sphx_gauge* __restrict__ tab, uint32_t n_gauges, const float* __restrict__ values,
                                                           float iso, uint32_t* __restrict__ out) {
    const uint32_t gi = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (gi >= n_gauges) return;  // (wavefront-uniform)
    const sphx_gauge g = tab[gi];
    const uint32_t lo = g.reserved[GAUGE_LO], cnt = g.reserved[GAUGE_CNT];
    const float* const f = values + g.reserved[GAUGE_OFF];
    uint32_t first = SPHX_GAUGE_NONE, last = SPHX_GAUGE_NONE, inside = 0, owned = 0;
    for (uint32_t k0 = 0; k0 < cnt; k0 += 64u) {
        const uint32_t k = k0 + lane;
        bool own = false, b = false;
        if (k < cnt) {  // (a lane behind the interval loads nothing)
            const float qx = g.x0 + (float)(lo + k) * g.dx;
            const float qy = g.y0 + (float)(lo + k) * g.dy;
            uint32_t cx, cy;
            cell_of(K, make_float2(qx, qy), cx, cy);
            own = rect_has(K.tile, cx, cy, 0u);
            b = own && f[k] >= iso;  // (NaN: outside)
        }
        owned += (uint32_t)__popcll(__ballot(own));
        const unsigned long long m = __ballot(b);
        if (m) {
            if (!inside) first = lo + k0 + (uint32_t)__ffsll((long long)m) - 1u;
            last = lo + k0 + 63u - (uint32_t)__clzll((long long)m);
            inside += (uint32_t)__popcll(m);
        }
    }
    if (lane != 0u) return;
    const uint32_t none = sphx_gauge_host::QNAN_WORD;
    uint32_t* const o = out + 8 * (size_t)gi;
    o[0] = lo, o[1] = owned, o[2] = first, o[3] = last, o[4] = inside;
    o[5] = cnt ? __float_as_uint(f[0]) : none;
    o[6] = inside ? __float_as_uint(f[last - lo]) : none;
    o[7] = inside && last + 1u < lo + cnt ? __float_as_uint(f[last + 1u - lo]) : none;
}

// point probes of a tile's frame: slot i is point i.  The tile that owns the point's cell stores k_probe_points' record with the
// "answered" mark in reserved[0] (the read strips it); every other tile skips the walk and stores an all-zero slot.
template <int KIND>
__global__ __launch_bounds__(256) void k_tile_probe_points(Consts K, SampleArgs a, const float* __restrict__ xy, uint32_t m, uint4* __restrict__ rec) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool live = i < m;
    const uint32_t k = live ? i : m - 1u;  // (m > 0)
    const float qx = xy[2 * (size_t)k], qy = xy[2 * (size_t)k + 1];
    uint32_t cx, cy;
    cell_of(K, make_float2(qx, qy), cx, cy);
    const bool own = live && rect_has(K.tile, cx, cy, 0u);
    const SampleSums r = sample_walk<KIND, true, true, true>(K, a, qx, qy, own);
    if (!live) return;
    const float2 v = sample_velocity(r);
    rec[2 * (size_t)k] = own ? make_uint4(__float_as_uint(r.rho), __float_as_uint(r.frac), __float_as_uint(v.x), __float_as_uint(v.y)) : make_uint4(0u, 0u, 0u, 0u);
    rec[2 * (size_t)k + 1] = own ? make_uint4(r.cnt, 1u, 0u, 0u) : make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace sphx

// ---- launch layer and C ABI ----------------------------------------------------------------------------------------------------------
namespace {

constexpr uint64_t PROBE_REC_BYTES_MAX = 64ull << 20;  // a recording's device buffer
constexpr uint32_t PROBE_MAX_POINTS = 1u << 20;

template <int KIND, bool DEN>
void gauge_launch_sample(sphx_ctx* c, const sphx_gauge* d_tab, uint32_t n_gauges, uint32_t total, float* d_values) {
    hipStream_t st = c->stream;
    const SampleArgs a = sample_args(c, sphx_sample_out{});
    // algorithmic bytes per sample: the value, ~ (9 cells) x (8-byte table entry), as enqueue_sample_t counts them
    launch(c, "gauge_sample", (4.0 + 72.0) * total, [&] {
        hipLaunchKernelGGL((sphx::k_gauge_sample<KIND, DEN>), dim3((total + 255u) / 256u), dim3(256), 0, st, c->K, a, d_tab, n_gauges, total, d_values);
    });
}
template <int KIND>
void gauge_launch_kind(sphx_ctx* c, const sphx_gauge* d_tab, uint32_t n_gauges, uint32_t total, int field, float* d_values) {
    if (field == SPHX_GAUGE_FIELD_DENSITY) gauge_launch_sample<KIND, true>(c, d_tab, n_gauges, total, d_values);
    else gauge_launch_sample<KIND, false>(c, d_tab, n_gauges, total, d_values);
}

// both passes behind what is on the stream: n_gauges records to d_out, the values to d_values (both device; total = the table's samples,
// > 0); the sweep direction launch() toggles is put back, as in stats_enqueue.
void gauge_enqueue(sphx_ctx* c, const sphx_gauge* d_tab, uint32_t n_gauges, uint32_t total, int kind, int field, float iso, float* d_values,
                   uint32_t* d_out) {
    const uint32_t rev = c->K.rev;
    hipStream_t st = c->stream;
    if (kind == SPHX_KERNEL_WENDLAND_C2) gauge_launch_kind<SPHX_KERNEL_WENDLAND_C2>(c, d_tab, n_gauges, total, field, d_values);
    else if (kind == SPHX_KERNEL_POLY6) gauge_launch_kind<SPHX_KERNEL_POLY6>(c, d_tab, n_gauges, total, field, d_values);
    else gauge_launch_kind<SPHX_KERNEL_SPIKY>(c, d_tab, n_gauges, total, field, d_values);
    launch(c, "gauge_reduce", 4.0 * total + 64.0 * n_gauges, [&] {
        hipLaunchKernelGGL(sphx::k_gauge_reduce, dim3((n_gauges + 3u) / 4u), dim3(256), 0, st, d_tab, n_gauges, (const float*)d_values, iso, d_out);
    }, false);
    c->K.rev = rev;
}

void probe_enqueue_points(sphx_ctx* c, const float* d_xy, uint32_t m, int kind, uint32_t* d_rec) {
    const uint32_t rev = c->K.rev;
    hipStream_t st = c->stream;
    const SampleArgs a = sample_args(c, sphx_sample_out{});
    const dim3 grid((m + 255u) / 256u);
    launch(c, "probe_points", (8.0 + 32.0 + 72.0) * m, [&] {
        if (kind == SPHX_KERNEL_WENDLAND_C2) hipLaunchKernelGGL((sphx::k_probe_points<SPHX_KERNEL_WENDLAND_C2>), grid, dim3(256), 0, st, c->K, a, d_xy, m, (uint4*)d_rec);
        else if (kind == SPHX_KERNEL_POLY6) hipLaunchKernelGGL((sphx::k_probe_points<SPHX_KERNEL_POLY6>), grid, dim3(256), 0, st, c->K, a, d_xy, m, (uint4*)d_rec);
        else hipLaunchKernelGGL((sphx::k_probe_points<SPHX_KERNEL_SPIKY>), grid, dim3(256), 0, st, c->K, a, d_xy, m, (uint4*)d_rec);
    });
    c->K.rev = rev;
}

// the caller's gauges with the flat index of each gauge's first sample in reserved[GAUGE_OFF]
std::vector<sphx_gauge> gauge_table(const sphx_gauge* gauges, uint32_t n_gauges) {
    std::vector<sphx_gauge> tab(gauges, gauges + n_gauges);
    uint32_t at = 0;
    for (sphx_gauge& g : tab) {
        g.reserved[0] = g.reserved[1] = g.reserved[2] = 0u;
        g.reserved[sphx::GAUGE_OFF] = at;
        at += g.n;
    }
    return tab;
}

// ... onto the device, behind what is on the stream (ceil(n / 64) launches; a dam break's handful of gauges is one)
void gauge_put_table(sphx_ctx* c, const std::vector<sphx_gauge>& tab, sphx_gauge* d_tab) {
    hipStream_t st = c->stream;
    for (size_t k0 = 0; k0 < tab.size(); k0 += sphx::GAUGE_CHUNK) {
        const uint32_t count = (uint32_t)std::min<size_t>(tab.size() - k0, sphx::GAUGE_CHUNK);
        sphx::GaugeChunk ch{};
        std::memcpy(ch.g, tab.data() + k0, (size_t)count * sizeof(sphx_gauge));
        launch(c, "gauge_table", 64.0 * count, [&] { hipLaunchKernelGGL(sphx::k_gauge_table, dim3(1), dim3(64), 0, st, ch, count, d_tab + k0); }, false);
    }
}

// the argument checks the one-shot call and the recorder share (they name the argument); *total = the samples of all gauges
int gauge_check_args(sphx_ctx* c, const char* fn, const sphx_gauge* gauges, uint32_t n_gauges, int kind, int field, float iso, uint64_t* total) {
    if (const char* bad = sphx_gauge_host::check(gauges, n_gauges, iso, total)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, bad);
    if (kind != SPHX_KERNEL_WENDLAND_C2 && kind != SPHX_KERNEL_POLY6 && kind != SPHX_KERNEL_SPIKY)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "unknown kernel_kind");
    if (field != SPHX_GAUGE_FIELD_FRACTION && field != SPHX_GAUGE_FIELD_DENSITY) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "unknown field");
    return SPHX_OK;
}

int probe_check_ctx(sphx_ctx* c, const char* fn) {
    if (c->tile_mode)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not available on a tile context (its arrays hold ghosts and miss the particles other tiles own)");
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, fn, "between step_begin and step_finish (finish the step first)");
    return SPHX_OK;
}

void probe_drop_recording(sphx_ctx* c) {
    sphx_ctx::Probe& p = c->probe;
    dev_free(&p.fixed);
    dev_free(&p.rec);
    p.info.clear();
    p.info.shrink_to_fit();
    p.m_points = p.n_gauges = p.total = 0;
    p.recording = p.max_frames = p.every = p.frames = p.dropped = p.steps = 0;
}

// One frame behind the kernels of the step that has just finished (sphx_step_finish / sphx_wcsph_step_finish call this through
// probe_after_step when a recording is on).  Nothing comes back to the host.  A step that left no sampleable state (sample_ready != 2: a
// step over zero fluid particles runs no build) takes no frame and is counted in `dropped`.
void probe_take_frame(sphx_ctx* c, float dt) {
    sphx_ctx::Probe& p = c->probe;
    if (c->tile_mode) return;
    if (++p.steps % p.every) return;
    if (p.frames >= p.max_frames || !c->uploaded || c->sample_ready != 2u) {
        p.dropped += 1u;
        return;
    }
    const sphx_gauge* const d_tab = (const sphx_gauge*)p.fixed;
    float* const d_values = (float*)(p.fixed + 8 * (size_t)p.n_gauges);
    const float* const d_xy = (const float*)(p.fixed + 8 * (size_t)p.n_gauges + p.total);
    uint32_t* const pts = p.rec + 8 * (size_t)p.m_points * p.frames;
    uint32_t* const gau = p.rec + 8 * (size_t)p.m_points * p.max_frames + 8 * (size_t)p.n_gauges * p.frames;
    if (p.m_points) probe_enqueue_points(c, d_xy, p.m_points, p.kind, pts);
    if (p.n_gauges) gauge_enqueue(c, d_tab, p.n_gauges, p.total, p.kind, p.field, p.iso, d_values, gau);
    p.info.push_back(sphx_stats_frame{p.steps, dt, c->N});
    p.frames += 1u;
}

}  // namespace

extern "C" {

int sphx_gauge_levels(sphx_ctx* c, const sphx_gauge* gauges, uint32_t n_gauges, int kernel_kind, int field, float iso, uint32_t flags,
                      sphx_gauge_rec* out, float* values) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_gauge_levels";
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out is NULL");
    int rc;
    uint64_t total64;
    if ((rc = gauge_check_args(c, fn, gauges, n_gauges, kernel_kind, field, iso, &total64))) return rc;
    if (flags & ~(uint32_t)SPHX_GAUGE_DEVICE_POINTERS) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "unknown flags bits");
    const bool device = (flags & SPHX_GAUGE_DEVICE_POINTERS) != 0u;
    if (device && ((uintptr_t)out & 3u)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out (a device pointer) is not 4-byte aligned");
    if (device && values && ((uintptr_t)values & 3u)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "values (a device pointer) is not 4-byte aligned");
    if (c->tile_mode)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not available on a tile context (its arrays hold ghosts and miss the particles other tiles own)");
    if (n_gauges == 0) return SPHX_OK;
    if ((rc = sample_check_state(c, fn))) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t total = (uint32_t)total64;
    // scratch: table [8 n_gauges] | values [total] (unless the caller's device array takes them) | host path: records [8 n_gauges]
    sphx_ctx::Probe& p = c->probe;
    const size_t at_val = 8 * (size_t)n_gauges, n_val = device && values ? 0 : (size_t)total, at_rec = at_val + n_val;
    const size_t words = at_rec + (device ? 0 : 8 * (size_t)n_gauges);
    if (words > p.scratch_cap) {
        SPHX_HIP(c, hipStreamSynchronize(c->stream));  // (a queued call may still use the old scratch)
        if ((rc = dev_alloc(c, &p.scratch, words))) {
            p.scratch_cap = 0;
            return rc;
        }
        p.scratch_cap = words;
    }
    const std::vector<sphx_gauge> tab = gauge_table(gauges, n_gauges);
    hipStream_t st = c->stream;
    gauge_put_table(c, tab, (sphx_gauge*)p.scratch);
    float* const d_values = device && values ? values : (float*)(p.scratch + at_val);
    uint32_t* const d_out = device ? (uint32_t*)out : p.scratch + at_rec;
    gauge_enqueue(c, (const sphx_gauge*)p.scratch, n_gauges, total, kernel_kind, field, iso, d_values, d_out);
    if (device) return SPHX_OK;
    SPHX_HIP(c, hipMemcpyAsync(out, d_out, (size_t)n_gauges * sizeof(sphx_gauge_rec), hipMemcpyDeviceToHost, st));
    if (values) SPHX_HIP(c, hipMemcpyAsync(values, d_values, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    SPHX_HIP(c, hipStreamSynchronize(st));
    return SPHX_OK;
}

int sphx_gauge_reduce(const float* values, const sphx_gauge* gauges, uint32_t n_gauges, float iso, sphx_gauge_rec* out) {
    return sphx_gauge_host::reduce(values, gauges, n_gauges, iso, out);
}

int sphx_probe_record(sphx_ctx* c, const float* points_xy, uint32_t m_points, const sphx_gauge* gauges, uint32_t n_gauges, int kernel_kind,
                      int field, float iso, uint32_t max_frames, uint32_t every) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_probe_record";
    int rc;
    if ((rc = probe_check_ctx(c, fn))) return rc;
    uint64_t total64 = 0;
    if (max_frames) {  // (max_frames == 0 stops and frees, whatever the other arguments say)
        if (every == 0) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "every must be >= 1");
        if (m_points >= PROBE_MAX_POINTS) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "m_points must be < 2^20");
        if (m_points && !points_xy) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "points_xy is NULL with m_points > 0");
        if ((rc = gauge_check_args(c, fn, gauges, n_gauges, kernel_kind, field, iso, &total64))) return rc;
        if (m_points + n_gauges == 0) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "m_points + n_gauges is 0: nothing to record");
        if ((uint64_t)max_frames * (m_points + n_gauges) * 32ull > PROBE_REC_BYTES_MAX)
            return c->fail(SPHX_ERR_CAPACITY, fn, "max_frames * (m_points + n_gauges) records exceed 64 MiB");
    }
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));  // (a queued frame may still write the old buffer)
    probe_drop_recording(c);
    if (!max_frames) return SPHX_OK;
    sphx_ctx::Probe& p = c->probe;
    const uint32_t total = (uint32_t)total64;
    const size_t at_xy = 8 * (size_t)n_gauges + total;
    if ((rc = dev_alloc(c, &p.fixed, at_xy + 2 * (size_t)m_points))) return rc;
    if ((rc = dev_alloc(c, &p.rec, 8 * (size_t)max_frames * (m_points + n_gauges)))) {
        dev_free(&p.fixed);
        return rc;
    }
    const std::vector<sphx_gauge> tab = gauge_table(gauges, n_gauges);
    gauge_put_table(c, tab, (sphx_gauge*)p.fixed);
    if (m_points) SPHX_HIP(c, hipMemcpyAsync(p.fixed + at_xy, points_xy, 2 * (size_t)m_points * 4, hipMemcpyHostToDevice, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));  // (points and gauges are copied at the call)
    p.m_points = m_points, p.n_gauges = n_gauges, p.total = total;
    p.kind = kernel_kind, p.field = field, p.iso = iso;
    p.max_frames = max_frames;
    p.every = every;
    p.recording = 1u;
    return SPHX_OK;
}

int sphx_probe_get_status(const sphx_ctx* c, sphx_probe_status* out) {
    if (!c || !out) return SPHX_ERR_INVALID_ARGUMENT;
    const sphx_ctx::Probe& p = c->probe;
    std::memset(out, 0, sizeof(*out));
    out->m_points = p.m_points;
    out->n_gauges = p.n_gauges;
    out->recording = p.recording;
    out->max_frames = p.max_frames;
    out->every = p.every;
    out->frames = p.frames;
    out->dropped = p.dropped;
    return SPHX_OK;
}

int sphx_probe_read(sphx_ctx* c, uint32_t first_frame, uint32_t n_frames, sphx_probe_rec* points_out, sphx_gauge_rec* gauges_out,
                    sphx_stats_frame* info) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_probe_read";
    int rc;
    if ((rc = probe_check_ctx(c, fn))) return rc;
    const sphx_ctx::Probe& p = c->probe;
    if ((uint64_t)first_frame + n_frames > p.frames)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "first_frame + n_frames is beyond the frames recorded (sphx_probe_get_status)");
    if (n_frames == 0) return SPHX_OK;
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t* const pts = p.rec + 8 * (size_t)p.m_points * first_frame;
    const uint32_t* const gau = p.rec + 8 * (size_t)p.m_points * p.max_frames + 8 * (size_t)p.n_gauges * first_frame;
    if (points_out && p.m_points)
        SPHX_HIP(c, hipMemcpyAsync(points_out, pts, (size_t)n_frames * p.m_points * sizeof(sphx_probe_rec), hipMemcpyDeviceToHost, c->stream));
    if (gauges_out && p.n_gauges)
        SPHX_HIP(c, hipMemcpyAsync(gauges_out, gau, (size_t)n_frames * p.n_gauges * sizeof(sphx_gauge_rec), hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    if (info) std::memcpy(info, p.info.data() + first_frame, (size_t)n_frames * sizeof(sphx_stats_frame));
    return SPHX_OK;
}

}  // extern "C"

// ---- one tile of a tiled run: the seam sphx_multi_gauge_levels and the sphx_multi_probe_* recorder (sphx_tiles.cpp) are built on ---------
// Enqueue and fetch halves, like the sampling seam: the multi enqueues on every tile's stream first and then collects, so the tiles'
// passes overlap.  The buffers are sphx_ctx::probe's (sphx_gauge_levels and sphx_probe_* refuse a tile context, so nobody else uses
// them there).
namespace {

int tile_gauge_check(sphx_ctx* c, const char* fn) {
    if (!c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not a tile context (sphx_gauge_levels / sphx_probe_* serve a plain one)");
    return SPHX_OK;
}

// The tile's table: the caller's gauges with the interval of the samples this tile owns (sphx_gauge_window.hpp: four bisections per
// gauge) and its compact offset.  lo_count gets {lo, count} per gauge; returns the number of owned samples.
uint32_t tile_gauge_table(const sphx_ctx* c, const sphx_gauge* gauges, uint32_t n_gauges, std::vector<sphx_gauge>& tab, std::vector<uint32_t>& lo_count) {
    tab.assign(gauges, gauges + n_gauges);
    lo_count.resize(2 * (size_t)n_gauges);
    const TileRect& r = c->K.tile;
    uint32_t at = 0;
    for (uint32_t k = 0; k < n_gauges; ++k) {
        sphx_gauge& g = tab[k];
        const sphx_gauge_host::Interval iv =
            sphx_gauge_host::gauge_interval(g.x0, g.y0, g.dx, g.dy, g.n, c->K.gmin_x, c->K.gmin_y, c->K.cell_inv, r.x0, r.x1, r.y0, r.y1);
        g.reserved[sphx::GAUGE_OFF] = at;
        g.reserved[sphx::GAUGE_LO] = lo_count[2 * (size_t)k] = iv.lo;
        g.reserved[sphx::GAUGE_CNT] = lo_count[2 * (size_t)k + 1] = iv.count;
        at += iv.count;  // (<= the sum of n <= 2^24)
    }
    return at;
}

int tile_gauge_args(sphx_ctx* c, SampleArgs& a) {
    a = SampleArgs{(const float2*)c->posA, (const float2*)c->vel, (const float*)c->density, c->soff(), NbGrid{}, NbGrid{}, nullptr, nullptr, nullptr, nullptr};
    return tile_sample_grids(c, a.gd, a.gs);
}

template <int KIND>
void tile_gauge_launch_kind(sphx_ctx* c, const SampleArgs& a, const sphx_gauge* d_tab, uint32_t n_gauges, uint32_t owned, int field, float* d_values) {
    hipStream_t st = c->stream;
    const dim3 grid((owned + 255u) / 256u);
    launch(c, "tile_gauge_sample", (4.0 + 72.0) * owned, [&] {
        if (field == SPHX_GAUGE_FIELD_DENSITY)
            hipLaunchKernelGGL((sphx::k_tile_gauge_sample<KIND, true>), grid, dim3(256), 0, st, c->K, a, d_tab, n_gauges, owned, d_values);
        else
            hipLaunchKernelGGL((sphx::k_tile_gauge_sample<KIND, false>), grid, dim3(256), 0, st, c->K, a, d_tab, n_gauges, owned, d_values);
    });
}

// both passes behind what is on the stream: n_gauges parts to d_parts, the owned samples' values to d_values (compact).  A tile that
// owns no sample runs the reduce pass alone (it stores the empty parts).  The sweep direction launch() toggles is put back.
void tile_gauge_enqueue(sphx_ctx* c, const SampleArgs& a, const sphx_gauge* d_tab, uint32_t n_gauges, uint32_t owned, int kind, int field, float iso,
                        float* d_values, uint32_t* d_parts) {
    const uint32_t rev = c->K.rev;
    hipStream_t st = c->stream;
    if (owned) {
        if (kind == SPHX_KERNEL_WENDLAND_C2) tile_gauge_launch_kind<SPHX_KERNEL_WENDLAND_C2>(c, a, d_tab, n_gauges, owned, field, d_values);
        else if (kind == SPHX_KERNEL_POLY6) tile_gauge_launch_kind<SPHX_KERNEL_POLY6>(c, a, d_tab, n_gauges, owned, field, d_values);
        else tile_gauge_launch_kind<SPHX_KERNEL_SPIKY>(c, a, d_tab, n_gauges, owned, field, d_values);
    }
    launch(c, "tile_gauge_reduce", 4.0 * owned + 64.0 * n_gauges, [&] {
        hipLaunchKernelGGL(sphx::k_tile_gauge_reduce, dim3((n_gauges + 3u) / 4u), dim3(256), 0, st, c->K, d_tab, n_gauges, (const float*)d_values, iso, d_parts);
    }, false);
    c->K.rev = rev;
}

void tile_probe_enqueue_points(sphx_ctx* c, const SampleArgs& a, const float* d_xy, uint32_t m, int kind, uint32_t* d_rec) {
    const uint32_t rev = c->K.rev;
    hipStream_t st = c->stream;
    const dim3 grid((m + 255u) / 256u);
    launch(c, "tile_probe_points", (8.0 + 32.0 + 72.0) * m, [&] {
        if (kind == SPHX_KERNEL_WENDLAND_C2) hipLaunchKernelGGL((sphx::k_tile_probe_points<SPHX_KERNEL_WENDLAND_C2>), grid, dim3(256), 0, st, c->K, a, d_xy, m, (uint4*)d_rec);
        else if (kind == SPHX_KERNEL_POLY6) hipLaunchKernelGGL((sphx::k_tile_probe_points<SPHX_KERNEL_POLY6>), grid, dim3(256), 0, st, c->K, a, d_xy, m, (uint4*)d_rec);
        else hipLaunchKernelGGL((sphx::k_tile_probe_points<SPHX_KERNEL_SPIKY>), grid, dim3(256), 0, st, c->K, a, d_xy, m, (uint4*)d_rec);
    });
    c->K.rev = rev;
}

// the device's counts against the host's intervals: a part that disagrees never reaches the fold
const char* tile_gauge_parts_check(const sphx_gauge_part* parts, const uint32_t* lo_count, size_t n) {
    for (size_t k = 0; k < n; ++k)
        if (parts[k].lo != lo_count[2 * k] || parts[k].count != lo_count[2 * k + 1])
            return "the device's ownership test disagrees with the host's interval of a gauge";
    return nullptr;
}

void tile_probe_drop_recording(sphx_ctx* c) {
    probe_drop_recording(c);
    sphx_ctx::Probe& p = c->probe;
    p.gauges_host.clear();
    p.table_lo_count.clear();
    p.frame_lo_count.clear();
    p.frame_lo_count.shrink_to_fit();
    p.table_valid = false;
    p.table_owned = 0;
}

}  // namespace

extern "C" {

int sphx_tile_gauge_levels(sphx_ctx* c, const sphx_gauge* gauges, uint32_t n_gauges, int kernel_kind, int field, float iso) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_gauge_levels";
    int rc;
    uint64_t total64;
    if ((rc = gauge_check_args(c, fn, gauges, n_gauges, kernel_kind, field, iso, &total64))) return rc;
    if ((rc = tile_gauge_check(c, fn))) return rc;
    sphx_ctx::Probe& p = c->probe;
    p.shot_gauges = 0;
    if (n_gauges == 0) return SPHX_OK;
    if ((rc = tile_sample_state(c, fn))) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    std::vector<sphx_gauge> tab;
    const uint32_t owned = tile_gauge_table(c, gauges, n_gauges, tab, p.shot_lo_count);
    // scratch: table [8 n_gauges] | parts [8 n_gauges] | compact values [owned]
    const size_t words = 16 * (size_t)n_gauges + owned;
    if (words > p.scratch_cap) {
        SPHX_HIP(c, hipStreamSynchronize(c->stream));  // (a queued call may still use the old scratch)
        if ((rc = dev_alloc(c, &p.scratch, words))) {
            p.scratch_cap = 0;
            return rc;
        }
        p.scratch_cap = words;
    }
    SampleArgs a;
    if ((rc = tile_gauge_args(c, a))) return rc;
    gauge_put_table(c, tab, (sphx_gauge*)p.scratch);
    tile_gauge_enqueue(c, a, (const sphx_gauge*)p.scratch, n_gauges, owned, kernel_kind, field, iso, (float*)(p.scratch + 16 * (size_t)n_gauges),
                       p.scratch + 8 * (size_t)n_gauges);
    p.shot_gauges = n_gauges;
    p.shot_owned = owned;
    return SPHX_OK;
}

int sphx_tile_gauge_fetch(sphx_ctx* c, sphx_gauge_part* parts, float* values, uint32_t* out_lo_count) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_gauge_fetch";
    int rc;
    if ((rc = tile_gauge_check(c, fn))) return rc;
    sphx_ctx::Probe& p = c->probe;
    const uint32_t n_gauges = p.shot_gauges, owned = p.shot_owned;
    if (!n_gauges) return SPHX_OK;  // (an empty call, or none: nothing was queued)
    if (!parts) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "parts is NULL");
    p.shot_gauges = 0;
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipMemcpyAsync(parts, p.scratch + 8 * (size_t)n_gauges, (size_t)n_gauges * sizeof(sphx_gauge_part), hipMemcpyDeviceToHost, c->stream));
    if (values && owned) SPHX_HIP(c, hipMemcpyAsync(values, p.scratch + 16 * (size_t)n_gauges, (size_t)owned * 4, hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    if (out_lo_count) std::memcpy(out_lo_count, p.shot_lo_count.data(), 2 * (size_t)n_gauges * 4);
    if (const char* bad = tile_gauge_parts_check(parts, p.shot_lo_count.data(), n_gauges)) return c->fail(SPHX_ERR_HIP, fn, bad);
    return SPHX_OK;
}

int sphx_tile_probe_record(sphx_ctx* c, const float* points_xy, uint32_t m_points, const sphx_gauge* gauges, uint32_t n_gauges, int kernel_kind,
                           int field, float iso, uint32_t max_frames, uint32_t every) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_probe_record";
    int rc;
    if ((rc = tile_gauge_check(c, fn))) return rc;
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, fn, "between step_begin and step_finish (finish the step first)");
    uint64_t total64 = 0;
    if (max_frames) {  // (max_frames == 0 stops and frees, whatever the other arguments say)
        if (every == 0) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "every must be >= 1");
        if (m_points >= PROBE_MAX_POINTS) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "m_points must be < 2^20");
        if (m_points && !points_xy) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "points_xy is NULL with m_points > 0");
        if ((rc = gauge_check_args(c, fn, gauges, n_gauges, kernel_kind, field, iso, &total64))) return rc;
        if (m_points + n_gauges == 0) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "m_points + n_gauges is 0: nothing to record");
        if ((uint64_t)max_frames * (m_points + n_gauges) * 32ull > PROBE_REC_BYTES_MAX)
            return c->fail(SPHX_ERR_CAPACITY, fn, "max_frames * (m_points + n_gauges) records exceed 64 MiB");
    }
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));  // (a queued frame may still write the old buffer)
    tile_probe_drop_recording(c);
    if (!max_frames) return SPHX_OK;
    sphx_ctx::Probe& p = c->probe;
    const uint32_t total = (uint32_t)total64;
    // fixed: table [8 n_gauges] | compact values [total: what the tile owns never exceeds it] | points [2 m_points]
    const size_t at_xy = 8 * (size_t)n_gauges + total;
    if ((rc = dev_alloc(c, &p.fixed, at_xy + 2 * (size_t)m_points))) return rc;
    if ((rc = dev_alloc(c, &p.rec, 8 * (size_t)max_frames * (m_points + n_gauges)))) {
        dev_free(&p.fixed);
        return rc;
    }
    if (m_points) SPHX_HIP(c, hipMemcpyAsync(p.fixed + at_xy, points_xy, 2 * (size_t)m_points * 4, hipMemcpyHostToDevice, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));  // (points and gauges are copied at the call)
    p.gauges_host.assign(gauges, gauges + n_gauges);
    p.m_points = m_points, p.n_gauges = n_gauges, p.total = total;
    p.kind = kernel_kind, p.field = field, p.iso = iso;
    p.max_frames = max_frames;
    p.every = every;
    p.recording = 1u;
    return SPHX_OK;
}

int sphx_tile_probe_due(const sphx_ctx* c) {
    if (!c || !c->tile_mode) return 0;
    const sphx_ctx::Probe& p = c->probe;
    return p.recording && (p.steps + 1u) % p.every == 0u && p.frames < p.max_frames ? 1 : 0;
}

// The tile loop calls this at the end of every finished step: with a recording on, every `every`-th call queues one frame behind the
// step's kernels.  The interval table follows the cuts: it is rebuilt on the host and sent again (kernel arguments) whenever the owned
// rectangle is not the one the table was built for.  Nothing comes back to the host and nothing is waited for.
int sphx_tile_probe_frame(sphx_ctx* c, float dt, uint32_t n_global) {
    if (!c || !c->tile_mode) return SPHX_ERR_INVALID_ARGUMENT;
    sphx_ctx::Probe& p = c->probe;
    if (!p.recording) return SPHX_OK;
    if (++p.steps % p.every) return SPHX_OK;
    if (p.frames >= p.max_frames || c->in_step || !c->lists_current || c->tile_pending_dt > 0.0f || !c->tile_density_ready || c->boundary_changed) {
        p.dropped += 1u;  // (beyond max_frames, or a step that left no sampleable state)
        return SPHX_OK;
    }
    SPHX_HIP(c, hipSetDevice(c->device));
    int rc;
    SampleArgs a;
    if ((rc = tile_gauge_args(c, a))) return rc;
    sphx_gauge* const d_tab = (sphx_gauge*)p.fixed;
    float* const d_values = (float*)(p.fixed + 8 * (size_t)p.n_gauges);
    const float* const d_xy = (const float*)(p.fixed + 8 * (size_t)p.n_gauges + p.total);
    uint32_t* const pts = p.rec + 8 * (size_t)p.m_points * p.frames;
    uint32_t* const gau = p.rec + 8 * (size_t)p.m_points * p.max_frames + 8 * (size_t)p.n_gauges * p.frames;
    if (p.m_points) tile_probe_enqueue_points(c, a, d_xy, p.m_points, p.kind, pts);
    if (p.n_gauges) {
        const TileRect& r = c->K.tile;
        if (!p.table_valid || p.table_rect[0] != r.x0 || p.table_rect[1] != r.x1 || p.table_rect[2] != r.y0 || p.table_rect[3] != r.y1) {
            std::vector<sphx_gauge> tab;
            p.table_owned = tile_gauge_table(c, p.gauges_host.data(), p.n_gauges, tab, p.table_lo_count);
            gauge_put_table(c, tab, d_tab);  // (behind the earlier frames' passes on the stream, which read the old table)
            p.table_rect[0] = r.x0, p.table_rect[1] = r.x1, p.table_rect[2] = r.y0, p.table_rect[3] = r.y1;
            p.table_valid = true;
        }
        tile_gauge_enqueue(c, a, d_tab, p.n_gauges, p.table_owned, p.kind, p.field, p.iso, d_values, gau);
        p.frame_lo_count.insert(p.frame_lo_count.end(), p.table_lo_count.begin(), p.table_lo_count.end());
    }
    p.info.push_back(sphx_stats_frame{p.steps, dt, n_global});
    p.frames += 1u;
    return SPHX_OK;
}

int sphx_tile_probe_read(sphx_ctx* c, uint32_t first_frame, uint32_t n_frames, sphx_probe_rec* points_out, sphx_gauge_part* parts_out,
                         sphx_stats_frame* info) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_probe_read";
    int rc;
    if ((rc = tile_gauge_check(c, fn))) return rc;
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, fn, "between step_begin and step_finish (finish the step first)");
    const sphx_ctx::Probe& p = c->probe;
    if ((uint64_t)first_frame + n_frames > p.frames)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "first_frame + n_frames is beyond the frames recorded (sphx_probe_get_status)");
    if (n_frames == 0) return SPHX_OK;
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t* const pts = p.rec + 8 * (size_t)p.m_points * first_frame;
    const uint32_t* const gau = p.rec + 8 * (size_t)p.m_points * p.max_frames + 8 * (size_t)p.n_gauges * first_frame;
    if (points_out && p.m_points)
        SPHX_HIP(c, hipMemcpyAsync(points_out, pts, (size_t)n_frames * p.m_points * sizeof(sphx_probe_rec), hipMemcpyDeviceToHost, c->stream));
    if (parts_out && p.n_gauges)
        SPHX_HIP(c, hipMemcpyAsync(parts_out, gau, (size_t)n_frames * p.n_gauges * sizeof(sphx_gauge_part), hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    if (info) std::memcpy(info, p.info.data() + first_frame, (size_t)n_frames * sizeof(sphx_stats_frame));
    if (parts_out && p.n_gauges)
        if (const char* bad = tile_gauge_parts_check(parts_out, p.frame_lo_count.data() + 2 * (size_t)p.n_gauges * first_frame, (size_t)n_frames * p.n_gauges))
            return c->fail(SPHX_ERR_HIP, fn, bad);
    return SPHX_OK;
}

}  // extern "C"
