// sphx_contour.inc — the iso-contour of a sampled field as directed segments (sphx_surface_contour) and the host stitcher
// (sphx_contour_chain); the contract is in include/sphx.h, "free-surface extraction", restated bit for bit by tests/contour_reference.py.
// Included at the end of sphx_kernels.hip behind sphx_sample.inc: pass (a) IS the lattice path of sphx_sample_grid (enqueue_sample with
// one output), so the values are that call's bits by construction.  Passes (b)-(d), one lane per cell, 256 cells per workgroup:
//   k_contour_count  classifies its cells and stores the workgroup's number of segments;
//   k_contour_carry  one workgroup turns those totals into exclusive offsets, chunk after chunk in ascending order, and stores *count;
//   k_contour_emit   classifies again (four loads from rows the count pass just read), scans its 256 counts and stores the segments.
// No atomic anywhere: an index is offset-of-workgroup + prefix-in-workgroup, both fixed by the cell order.  Compiled with
// -ffp-contract=off like the rest: the crossing point's operations are rounded one by one.

#include "sphx_contour_chain.hpp"

namespace sphx {

struct ContourLattice {
    float x0, y0, dx, dy, iso;
    uint32_t nx, cx, cells;  // cx = nx - 1 cells per row, cells = cx * (ny - 1) < 2^31
};
constexpr uint32_t CONTOUR_MAX_BLOCKS = 1u << 22;  // workgroups per launch, as SAMPLE_MAX_BLOCKS

// edges in the contract's order, and per case the segment as (from | to << 2); the saddles (5, 10) are resolved by the centre
constexpr uint32_t CE_B = 0, CE_R = 1, CE_T = 2, CE_L = 3;
constexpr uint64_t contour_nib(uint32_t c, uint32_t from, uint32_t to) { return (uint64_t)(from | to << 2) << (4u * c); }
constexpr uint64_t CONTOUR_SEG = contour_nib(1, CE_B, CE_L) | contour_nib(2, CE_R, CE_B) | contour_nib(4, CE_T, CE_R) | contour_nib(8, CE_L, CE_T) |
                                 contour_nib(3, CE_R, CE_L) | contour_nib(6, CE_T, CE_B) | contour_nib(12, CE_L, CE_R) | contour_nib(9, CE_B, CE_T) |
                                 contour_nib(14, CE_L, CE_B) | contour_nib(13, CE_B, CE_R) | contour_nib(11, CE_R, CE_T) | contour_nib(7, CE_T, CE_L);
constexpr uint32_t contour_pair(uint32_t f0, uint32_t t0, uint32_t f1, uint32_t t1) { return (f0 | t0 << 2) | (f1 | t1 << 2) << 4; }
constexpr uint32_t CONTOUR_5_IN = contour_pair(CE_B, CE_R, CE_T, CE_L), CONTOUR_5_OUT = contour_pair(CE_B, CE_L, CE_T, CE_R);
constexpr uint32_t CONTOUR_10_IN = contour_pair(CE_R, CE_T, CE_L, CE_B), CONTOUR_10_OUT = contour_pair(CE_R, CE_B, CE_L, CE_T);

struct ContourCell {
    float f0, f1, f2, f3;
    uint32_t ix, iy;
    uint32_t n;     // segments: 0, 1 or 2
    uint32_t segs;  // segment k in bits [4k, 4k + 4): from | to << 2
};
// cell `cell` (< L.cells) of the lattice of values f: the four nodes (two loads from each of two rows), the case and its segments
__device__ __forceinline__ ContourCell contour_classify(const ContourLattice& L, const float* __restrict__ f, uint32_t cell) {
    ContourCell r;
    r.iy = cell / L.cx;
    r.ix = cell - r.iy * L.cx;
    const size_t at = (size_t)r.iy * L.nx + r.ix;
    r.f0 = f[at], r.f1 = f[at + 1], r.f3 = f[at + L.nx], r.f2 = f[at + L.nx + 1];
    const uint32_t c = (r.f0 >= L.iso ? 1u : 0u) | (r.f1 >= L.iso ? 2u : 0u) | (r.f2 >= L.iso ? 4u : 0u) | (r.f3 >= L.iso ? 8u : 0u);  // (NaN: outside)
    if (c == 5u || c == 10u) {
        const bool in = ((r.f0 + r.f1) + (r.f2 + r.f3)) * 0.25f >= L.iso;
        r.n = 2u;
        r.segs = c == 5u ? (in ? CONTOUR_5_IN : CONTOUR_5_OUT) : (in ? CONTOUR_10_IN : CONTOUR_10_OUT);
    } else {
        r.n = (c == 0u || c == 15u) ? 0u : 1u;
        r.segs = (uint32_t)(CONTOUR_SEG >> (4u * c)) & 15u;
    }
    return r;
}
// the crossing point of edge e of the cell: a = the node of the lower lattice index, b = the other; every operation rounded once
__device__ __forceinline__ float2 contour_cross(const ContourLattice& L, const ContourCell& q, uint32_t e) {
    const float xl = L.x0 + (float)q.ix * L.dx, xr = L.x0 + (float)(q.ix + 1u) * L.dx;
    const float yb = L.y0 + (float)q.iy * L.dy, yt = L.y0 + (float)(q.iy + 1u) * L.dy;
    const float xa = e == CE_R ? xr : xl, ya = e == CE_T ? yt : yb;
    const float xb = e == CE_L ? xl : xr, yb2 = e == CE_B ? yb : yt;
    const float fa = e == CE_R ? q.f1 : (e == CE_T ? q.f3 : q.f0);
    const float fb = e == CE_B ? q.f1 : (e == CE_L ? q.f3 : q.f2);
    const float t = (L.iso - fa) / (fb - fa);
    return make_float2(xa + t * (xb - xa), ya + t * (yb2 - ya));
}

// (b) + the workgroup's total.  Workgroup base + blockIdx.x owns the cells [256 b, 256 b + 256).
__global__ __launch_bounds__(256) void k_contour_count(ContourLattice L, const float* __restrict__ f, uint32_t* __restrict__ block_total, uint32_t base) {
    const uint32_t b = base + blockIdx.x, cell = b * 256u + threadIdx.x;
    const uint32_t n = cell < L.cells ? contour_classify(L, f, cell).n : 0u;
    uint32_t total;
    block_excl_scan_256(n, &total);
    if (threadIdx.x == 0) block_total[b] = total;
}
// (c) across workgroups: ONE workgroup walks the totals in chunks of 256 in ascending order and replaces each by the sum of all before
// it; the grand total goes to *count.  (2 * cells < 2^32: the sums fit.)
__global__ __launch_bounds__(256) void k_contour_carry(uint32_t* __restrict__ block_total, uint32_t nblocks, uint32_t* __restrict__ count) {
    uint32_t carry = 0;
    for (uint32_t i0 = 0; i0 < nblocks; i0 += 256u) {  // (workgroup-uniform bounds)
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t v = i < nblocks ? block_total[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_scan_256(v, &total);
        if (i < nblocks) block_total[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) count[0] = carry;
}
// (c) inside the workgroup + (d): segment index = the workgroup's offset + the exclusive prefix of the lane's count; one 16-byte store per
// segment below the capacity, and its cell word.
__global__ __launch_bounds__(256) void k_contour_emit(ContourLattice L, const float* __restrict__ f, const uint32_t* __restrict__ block_off, uint32_t cap,
                                                      float4* __restrict__ seg, uint32_t* __restrict__ cell_out, uint32_t base) {
    const uint32_t b = base + blockIdx.x, cell = b * 256u + threadIdx.x;
    ContourCell q{};
    if (cell < L.cells) q = contour_classify(L, f, cell);
    uint32_t total;
    const uint32_t ex = block_excl_scan_256(q.n, &total);
    const uint32_t first = block_off[b] + ex;
#pragma unroll
    for (uint32_t k = 0; k < 2u; ++k) {
        const uint32_t at = first + k;
        if (k < q.n && at < cap) {
            if (seg) {
                const uint32_t s = q.segs >> (4u * k);
                const float2 p0 = contour_cross(L, q, s & 3u), p1 = contour_cross(L, q, (s >> 2) & 3u);
                seg[at] = make_float4(p0.x, p0.y, p1.x, p1.y);
            }
            if (cell_out) cell_out[at] = cell;
        }
    }
}

}  // namespace sphx

// ---- launch layer and C ABI ----------------------------------------------------------------------------------------------------------
namespace {

// scratch of sphx_surface_contour in 4-byte words, grown on demand (the stream is drained before the old one is freed)
int contour_scratch(sphx_ctx* c, size_t words) {
    if (words <= c->contour_cap && c->contour_buf) return SPHX_OK;
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    int rc;
    if ((rc = dev_alloc(c, &c->contour_buf, words))) {
        c->contour_cap = 0;
        return rc;
    }
    c->contour_cap = words;
    return SPHX_OK;
}

}  // namespace

extern "C" {

int sphx_surface_contour(sphx_ctx* c, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, int kernel_kind, int field, float iso,
                         uint32_t cap_segments, uint32_t flags, const sphx_contour_out* out) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_surface_contour";
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out is NULL");
    if (!out->count) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out->count is NULL");
    if (kernel_kind != SPHX_KERNEL_WENDLAND_C2 && kernel_kind != SPHX_KERNEL_POLY6 && kernel_kind != SPHX_KERNEL_SPIKY)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "unknown kernel_kind");
    if (field != SPHX_CONTOUR_FIELD_FRACTION && field != SPHX_CONTOUR_FIELD_DENSITY) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "unknown field");
    if (flags & ~(uint32_t)SPHX_CONTOUR_DEVICE_POINTERS) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "unknown flags bits");
    if (!std::isfinite(iso)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "iso must be finite");
    if (c->tile_mode)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not available on a tile context (its arrays hold ghosts and miss the particles other tiles own)");
    if (!std::isfinite(x0) || !std::isfinite(y0)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "x0 / y0 must be finite");
    if (!std::isfinite(dx) || !(dx > 0.0f)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "dx must be finite and > 0");
    if (!std::isfinite(dy) || !(dy > 0.0f)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "dy must be finite and > 0");
    const uint64_t m = (uint64_t)nx * ny;
    if (m >= (1ull << 31)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "nx * ny must be < 2^31");
    const bool device = (flags & SPHX_CONTOUR_DEVICE_POINTERS) != 0u;
    if (device && out->segments && ((uintptr_t)out->segments & 15u))
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out->segments must be 16-byte aligned (a segment is one 16-byte store)");
    if (m == 0) {  // (as sphx_sample_grid: an empty lattice is a no-op once the arguments pass)
        if (!device) {
            out->count[0] = 0u;
            return SPHX_OK;
        }
        SPHX_HIP(c, hipSetDevice(c->device));
        SPHX_HIP(c, hipMemsetAsync(out->count, 0, 4, c->stream));
        return SPHX_OK;
    }
    int rc;
    if ((rc = sample_check_state(c, fn))) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t cells = nx >= 2u && ny >= 2u ? (nx - 1u) * (ny - 1u) : 0u;
    const uint32_t nblocks = (cells + 255u) / 256u;
    const uint32_t cap = (uint32_t)std::min<uint64_t>(cap_segments, 2ull * cells);  // (a cell emits two at most: nothing above is ever written)
    const bool want_seg = out->segments != nullptr && cap > 0u, want_cell = out->cell != nullptr && cap > 0u;
    if (!cells && !out->values) {  // one row or one column: no cell, and nobody asked for the values
        if (device) SPHX_HIP(c, hipMemsetAsync(out->count, 0, 4, c->stream));
        else out->count[0] = 0u;
        return SPHX_OK;
    }
    // scratch: values [m] (unless the caller's device array takes them) | offsets [nblocks] | host path: count [1], pad to 16 bytes,
    // segments [4 cap], cells [cap]
    const size_t at_val = 0, n_val = device && out->values ? 0 : (size_t)m;
    const size_t at_off = at_val + n_val, at_cnt = at_off + nblocks, at_seg = (at_cnt + 1u + 3u) & ~(size_t)3u;
    const size_t at_cell = at_seg + (device || !want_seg ? 0 : 4 * (size_t)cap);
    const size_t words = device ? at_cnt : at_cell + (want_cell ? (size_t)cap : 0);
    if ((rc = contour_scratch(c, std::max<size_t>(words, 1)))) return rc;
    uint32_t* const buf = (uint32_t*)c->contour_buf;
    float* const d_val = device && out->values ? out->values : (float*)(buf + at_val);
    uint32_t* const d_off = buf + at_off;
    uint32_t* const d_cnt = device ? out->count : buf + at_cnt;
    float4* const d_seg = !want_seg ? nullptr : (device ? (float4*)out->segments : (float4*)(buf + at_seg));
    uint32_t* const d_cell = !want_cell ? nullptr : (device ? out->cell : buf + at_cell);
    hipStream_t st = c->stream;
    const uint32_t rev = c->K.rev;  // (launch() toggles the sweep direction of the step's next kernels: put back below)
    // (a) the lattice values: sphx_sample_grid's own launch with the one output
    {
        const sphx::SampleLattice SL{x0, y0, dx, dy, nx, ny, (nx + sphx::SAMPLE_TILE - 1) / sphx::SAMPLE_TILE};
        sphx_sample_out so{};
        const bool den = field == SPHX_CONTOUR_FIELD_DENSITY;
        (den ? so.density : so.fraction) = d_val;
        enqueue_sample(c, SampleJob{nullptr, 0, &SL, sample_args(c, so)}, kernel_kind, den ? SAMPLE_OUT_DENSITY : SAMPLE_OUT_FRACTION, m);
    }
    if (!cells) {
        SPHX_HIP(c, hipMemsetAsync(d_cnt, 0, 4, st));
    } else {
        const sphx::ContourLattice L{x0, y0, dx, dy, iso, nx, nx - 1u, cells};
        for (uint32_t b0 = 0; b0 < nblocks; b0 += sphx::CONTOUR_MAX_BLOCKS) {
            const uint32_t nb = std::min(nblocks - b0, sphx::CONTOUR_MAX_BLOCKS);
            launch(c, "contour_count", 4.0 * (double)nb * 256.0 + 4.0 * nb, [&] {
                hipLaunchKernelGGL(sphx::k_contour_count, dim3(nb), dim3(256), 0, st, L, (const float*)d_val, d_off, b0);
            });
        }
        launch(c, "contour_carry", 8.0 * nblocks, [&] { hipLaunchKernelGGL(sphx::k_contour_carry, dim3(1), dim3(256), 0, st, d_off, nblocks, d_cnt); }, false);
        if (want_seg || want_cell) {
            for (uint32_t b0 = 0; b0 < nblocks; b0 += sphx::CONTOUR_MAX_BLOCKS) {
                const uint32_t nb = std::min(nblocks - b0, sphx::CONTOUR_MAX_BLOCKS);
                launch(c, "contour_emit", 4.0 * (double)nb * 256.0 + 4.0 * nb, [&] {
                    hipLaunchKernelGGL(sphx::k_contour_emit, dim3(nb), dim3(256), 0, st, L, (const float*)d_val, (const uint32_t*)d_off, cap, d_seg, d_cell, b0);
                });
            }
        }
    }
    c->K.rev = rev;
    if (device) return SPHX_OK;
    uint32_t total = 0;
    SPHX_HIP(c, hipMemcpyAsync(&total, d_cnt, 4, hipMemcpyDeviceToHost, st));
    if (out->values) SPHX_HIP(c, hipMemcpyAsync(out->values, d_val, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    SPHX_HIP(c, hipStreamSynchronize(st));
    out->count[0] = total;
    const size_t got = std::min<size_t>(total, cap);
    if (got && d_seg) SPHX_HIP(c, hipMemcpyAsync(out->segments, d_seg, got * 16, hipMemcpyDeviceToHost, st));
    if (got && d_cell) SPHX_HIP(c, hipMemcpyAsync(out->cell, d_cell, got * 4, hipMemcpyDeviceToHost, st));
    if (got) SPHX_HIP(c, hipStreamSynchronize(st));
    return SPHX_OK;
}

int sphx_contour_chain(const float* segments, uint32_t n, uint32_t* order, uint32_t* line_first, uint8_t* closed, uint32_t* out_lines) {
    if (!out_lines) return SPHX_ERR_INVALID_ARGUMENT;
    *out_lines = 0;
    if (n == 0) {
        if (line_first) line_first[0] = 0;
        return SPHX_OK;
    }
    if (!segments || !order || !line_first || !closed) return SPHX_ERR_INVALID_ARGUMENT;
    *out_lines = sphx_contour_host::chain(segments, n, order, line_first, closed);
    return SPHX_OK;
}

}  // extern "C"
