// sphx_contour.inc — the iso-contour of a sampled field as directed segments (sphx_surface_contour) and the host stitcher
// (sphx_contour_chain); the contract is in include/sphx.h, "free-surface extraction", restated bit for bit by tests/contour_reference.py.
// Included at the end of sphx_kernels.hip behind sphx_sample.inc: pass (a) IS the lattice path of sphx_sample_grid (enqueue_sample with
// one output), so the values are that call's bits by construction.  Passes (b)-(d), one lane per cell, 256 cells per workgroup:
//   k_contour_count  classifies its cells and stores the workgroup's number of segments;
//   k_contour_carry  one workgroup turns those totals into exclusive offsets, chunk after chunk in ascending order, and stores *count;
//   k_contour_emit   classifies again (four loads from rows the count pass just read), scans its 256 counts and stores the segments.
// No atomic anywhere: an index is offset-of-workgroup + prefix-in-workgroup, both fixed by the cell order.  Compiled with
// -ffp-contract=off like the rest: the crossing point's operations are rounded one by one.
// The same three kernels cut a tile's padded window of the lattice for sphx_multi_surface_contour (sphx_tile_contour_*, at the end).

#include "sphx_contour_chain.hpp"

namespace sphx {

// The cells the kernels walk form the rectangle [ix0, ix0 + cx) x [iy0, ...) of the lattice's cells, `cells` of them, over values stored
// `pitch` words per row with the rectangle's node (ix0, iy0) first.  sphx_surface_contour: the whole lattice (offset 0, pitch nx,
// gcx = cx).  sphx_tile_contour_cut: a tile's padded window.  Points and cell words are formed from the GLOBAL indices either way.
struct ContourLattice {
    float x0, y0, dx, dy, iso;
    uint32_t pitch, cx, cells;  // cx cells per row of the rectangle, cells = cx * rows < 2^31
    uint32_t ix0, iy0, gcx;     // the rectangle's first cell; gcx = nx - 1 of the whole lattice (the cell word is iy * gcx + ix)
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
    uint32_t ix, iy;  // global
    uint32_t word;    // iy * (nx - 1) + ix
    uint32_t n;     // segments: 0, 1 or 2
    uint32_t segs;  // segment k in bits [4k, 4k + 4): from | to << 2
};
// cell `cell` (< L.cells) of the rectangle, over the values f: the four nodes (two loads from each of two rows), the case and its segments
__device__ __forceinline__ ContourCell contour_classify(const ContourLattice& L, const float* __restrict__ f, uint32_t cell) {
    ContourCell r;
    const uint32_t ly = cell / L.cx, lx = cell - ly * L.cx;
    r.iy = L.iy0 + ly;
    r.ix = L.ix0 + lx;
    r.word = r.iy * L.gcx + r.ix;
    const size_t at = (size_t)ly * L.pitch + lx;
    r.f0 = f[at], r.f1 = f[at + 1], r.f3 = f[at + L.pitch], r.f2 = f[at + L.pitch + 1];
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
            if (cell_out) cell_out[at] = q.word;
        }
    }
}

// ---- one tile of a tiled run (sphx_tile_contour_*, include/sphx.h "free surface of a tiled run") ---------------------------------------
// A tile samples its window of the lattice into an array padded by one APRON column (ax) and row (ay) whose nodes other tiles own.
// Every apron node is in the first row or the first column of some tile's window, so the tiles swap those alone.

// row 0, then column 0 of the window's values (wnx x wny nodes, `pitch` words per row) as one run of wnx + wny words
__global__ __launch_bounds__(256) void k_contour_border_pack(const uint32_t* __restrict__ val, uint32_t wnx, uint32_t wny, uint32_t pitch,
                                                             uint32_t* __restrict__ border) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < wnx) border[i] = val[i];
    else if (i < wnx + wny) border[i] = val[(size_t)(i - wnx) * pitch];
}
// the apron into the padded array of (wnx + ax) x (wny + ay) words: apron = column wnx of rows [0, wny) if ax, then row wny of columns
// [0, wnx) if ay, then the corner (wnx, wny) if both
__global__ __launch_bounds__(256) void k_contour_apron_unpack(const uint32_t* __restrict__ apron, uint32_t wnx, uint32_t wny, uint32_t ax, uint32_t ay,
                                                              uint32_t pitch, uint32_t* __restrict__ val) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n_col = ax ? wny : 0u, n_row = ay ? wnx : 0u;
    if (i < n_col) val[(size_t)i * pitch + wnx] = apron[i];
    else if (i < n_col + n_row) val[(size_t)wny * pitch + (i - n_col)] = apron[i];
    else if (i < n_col + n_row + (ax & ay)) val[(size_t)wny * pitch + wnx] = apron[i];
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

// passes (b)-(d) over the cells of L on the context's stream: count, carry, and emit if an output is wanted
void contour_enqueue_cut(sphx_ctx* c, const sphx::ContourLattice& L, const float* d_val, uint32_t* d_off, uint32_t nblocks, uint32_t* d_cnt, uint32_t cap,
                         float4* d_seg, uint32_t* d_cell) {
    hipStream_t st = c->stream;
    for (uint32_t b0 = 0; b0 < nblocks; b0 += sphx::CONTOUR_MAX_BLOCKS) {
        const uint32_t nb = std::min(nblocks - b0, sphx::CONTOUR_MAX_BLOCKS);
        launch(c, "contour_count", 4.0 * (double)nb * 256.0 + 4.0 * nb, [&] {
            hipLaunchKernelGGL(sphx::k_contour_count, dim3(nb), dim3(256), 0, st, L, (const float*)d_val, d_off, b0);
        });
    }
    launch(c, "contour_carry", 8.0 * nblocks, [&] { hipLaunchKernelGGL(sphx::k_contour_carry, dim3(1), dim3(256), 0, st, d_off, nblocks, d_cnt); }, false);
    if (d_seg || d_cell) {
        for (uint32_t b0 = 0; b0 < nblocks; b0 += sphx::CONTOUR_MAX_BLOCKS) {
            const uint32_t nb = std::min(nblocks - b0, sphx::CONTOUR_MAX_BLOCKS);
            launch(c, "contour_emit", 4.0 * (double)nb * 256.0 + 4.0 * nb, [&] {
                hipLaunchKernelGGL(sphx::k_contour_emit, dim3(nb), dim3(256), 0, st, L, (const float*)d_val, (const uint32_t*)d_off, cap, d_seg, d_cell, b0);
            });
        }
    }
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
        const sphx::ContourLattice L{x0, y0, dx, dy, iso, nx, nx - 1u, cells, 0u, 0u, nx - 1u};
        contour_enqueue_cut(c, L, d_val, d_off, nblocks, d_cnt, cap, d_seg, d_cell);
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

// ---- one tile of a tiled run: sample the padded window + pack its border | fetch the border | unpack the apron + cut | fetch -----------
int sphx_tile_contour_sample(sphx_ctx* c, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, int kernel_kind, int field,
                             uint32_t* out_window) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_contour_sample";
    if (!out_window) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out_window is NULL");
    out_window[0] = out_window[1] = out_window[2] = out_window[3] = 0u;
    if (!c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not a tile context (sphx_surface_contour serves a plain one)");
    if (kernel_kind != SPHX_KERNEL_WENDLAND_C2 && kernel_kind != SPHX_KERNEL_POLY6 && kernel_kind != SPHX_KERNEL_SPIKY)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "unknown kernel_kind");
    if (field != SPHX_CONTOUR_FIELD_FRACTION && field != SPHX_CONTOUR_FIELD_DENSITY) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "unknown field");
    if (!std::isfinite(x0) || !std::isfinite(y0)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "x0 / y0 must be finite");
    if (!std::isfinite(dx) || !(dx > 0.0f)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "dx must be finite and > 0");
    if (!std::isfinite(dy) || !(dy > 0.0f)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "dy must be finite and > 0");
    if ((uint64_t)nx * ny >= (1ull << 31)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "nx * ny must be < 2^31");
    sphx_ctx::TileContour& T = c->tcontour;
    T = sphx_ctx::TileContour{};
    int rc;
    if ((uint64_t)nx * ny && (rc = tile_sample_state(c, fn))) return rc;
    T.stage = 1u;
    T.x0 = x0, T.y0 = y0, T.dx = dx, T.dy = dy, T.gcx = nx ? nx - 1u : 0u;
    if ((uint64_t)nx * ny == 0) return SPHX_OK;
    const sphx_sample_host::Window w = sphx_sample_host::lattice_window(x0, y0, dx, dy, nx, ny, c->K.gmin_x, c->K.gmin_y, c->K.cell_inv, c->K.tile.x0,
                                                                      c->K.tile.x1, c->K.tile.y0, c->K.tile.y1);
    if (!w.points()) return SPHX_OK;  // no lattice node falls into a cell this tile owns: no border, no cell to cut
    const uint32_t wnx = w.w(), wny = w.h();
    const uint32_t ax = w.ix1 < nx ? 1u : 0u, ay = w.iy1 < ny ? 1u : 0u;
    const uint32_t pitch = wnx + ax;
    const size_t n_val = (size_t)pitch * (wny + ay);
    const uint32_t cells = (wnx - 1u + ax) * (wny - 1u + ay);  // (< nx * ny < 2^31)
    const uint32_t nblocks = (cells + 255u) / 256u;
    // scratch: values [pitch * (wny + ay)] | border [wnx + wny] | apron [wnx + wny + 1] | offsets [nblocks]
    T.at_border = n_val, T.at_apron = T.at_border + wnx + wny, T.at_off = T.at_apron + wnx + wny + 1u;
    T.stage = 0u;
    SPHX_HIP(c, hipSetDevice(c->device));
    if ((rc = contour_scratch(c, T.at_off + nblocks))) return rc;
    const bool den = field == SPHX_CONTOUR_FIELD_DENSITY;
    SampleArgs a{(const float2*)c->posA, (const float2*)c->vel, (const float*)c->density, c->soff(), NbGrid{}, NbGrid{}, nullptr, nullptr, nullptr, nullptr};
    if ((rc = tile_sample_grids(c, a.gd, a.gs))) return rc;
    uint32_t* const buf = c->contour_buf;
    (den ? a.o_density : a.o_fraction) = (float*)buf;
    hipStream_t st = c->stream;
    SPHX_HIP(c, hipMemsetAsync(buf, 0, n_val * 4, st));  // (a lane that is not the owner writes nothing; the apron arrives in _cut)
    const SampleLattice L{x0, y0, dx, dy, nx, ny, (nx + SAMPLE_TILE - 1) / SAMPLE_TILE};
    const SampleWindow W{w.ix0, w.iy0, wnx, wny, (wnx + SAMPLE_TILE - 1) / SAMPLE_TILE, pitch};
    const uint32_t rev = c->K.rev;  // (launch() toggles the sweep direction of the step's next kernels: put back below)
    SampleJob q{nullptr, 0, &L, a};
    q.window = &W;
    enqueue_sample(c, q, kernel_kind, den ? SAMPLE_OUT_DENSITY : SAMPLE_OUT_FRACTION, w.points());
    const uint32_t nb = (wnx + wny + 255u) / 256u;
    launch(c, "contour_border_pack", 8.0 * (wnx + wny), [&] {
        hipLaunchKernelGGL(sphx::k_contour_border_pack, dim3(nb), dim3(256), 0, st, (const uint32_t*)buf, wnx, wny, pitch, buf + T.at_border);
    }, false);
    c->K.rev = rev;
    T.win[0] = out_window[0] = w.ix0, T.win[1] = out_window[1] = w.ix1, T.win[2] = out_window[2] = w.iy0, T.win[3] = out_window[3] = w.iy1;
    T.ax = ax, T.ay = ay, T.cells = cells, T.nblocks = nblocks;
    T.stage = 1u;
    return SPHX_OK;
}

int sphx_tile_contour_border_fetch(sphx_ctx* c, uint32_t* border, uint32_t cap_words) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_contour_border_fetch";
    if (!c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not a tile context");
    const sphx_ctx::TileContour& T = c->tcontour;
    if (T.stage != 1u) return c->fail(SPHX_ERR_NOT_READY, fn, "no sampled window is waiting (sphx_tile_contour_sample first)");
    const uint32_t n = (T.win[1] - T.win[0]) + (T.win[3] - T.win[2]);
    if (!n) return SPHX_OK;
    if (!border || cap_words < n) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "border is NULL or shorter than the window's row 0 + column 0");
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipMemcpyAsync(border, c->contour_buf + T.at_border, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    return SPHX_OK;
}

int sphx_tile_contour_cut(sphx_ctx* c, float iso, uint32_t cap_segments, const uint32_t* apron, uint32_t n_apron) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_contour_cut";
    if (!c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not a tile context");
    sphx_ctx::TileContour& T = c->tcontour;
    if (T.stage != 1u) return c->fail(SPHX_ERR_NOT_READY, fn, "no sampled window is waiting (sphx_tile_contour_sample first)");
    if (!std::isfinite(iso)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "iso must be finite");
    const uint32_t wnx = T.win[1] - T.win[0], wny = T.win[3] - T.win[2];
    const uint32_t need = wnx && wny ? (T.ax ? wny : 0u) + (T.ay ? wnx : 0u) + (T.ax & T.ay) : 0u;
    if (n_apron != need || (need && !apron)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "apron does not hold the window's last column, last row and corner");
    T.cap = (uint32_t)std::min<uint64_t>(cap_segments, 2ull * T.cells);  // (a cell emits two at most: nothing above is ever written)
    T.iso = iso;
    if (!T.cells) {  // nothing to cut (no node, or a window without a neighbour on one side that is one node wide or high)
        T.stage = 2u;
        return SPHX_OK;
    }
    SPHX_HIP(c, hipSetDevice(c->device));
    // the outputs' device copies live in the tile's sample scratch: count [1], pad to 16 bytes | segments [4 cap] | cells [cap]
    T.at_cnt = 0, T.at_seg = 4, T.at_cell = T.at_seg + 4 * (size_t)T.cap;
    int rc;
    if ((rc = tile_sample_scratch(c, T.at_cell + T.cap))) return rc;
    uint32_t* const buf = c->contour_buf;
    uint32_t* const obuf = (uint32_t*)c->sample_buf;
    hipStream_t st = c->stream;
    const uint32_t pitch = wnx + T.ax;
    const uint32_t rev = c->K.rev;
    if (need) {
        SPHX_HIP(c, hipMemcpyAsync(buf + T.at_apron, apron, (size_t)need * 4, hipMemcpyHostToDevice, st));
        const uint32_t nb = (need + 255u) / 256u;
        launch(c, "contour_apron_unpack", 8.0 * need, [&] {
            hipLaunchKernelGGL(sphx::k_contour_apron_unpack, dim3(nb), dim3(256), 0, st, (const uint32_t*)(buf + T.at_apron), wnx, wny, T.ax, T.ay, pitch, buf);
        }, false);
    }
    const sphx::ContourLattice L{T.x0, T.y0, T.dx, T.dy, iso, pitch, wnx - 1u + T.ax, T.cells, T.win[0], T.win[2], T.gcx};
    contour_enqueue_cut(c, L, (const float*)buf, buf + T.at_off, T.nblocks, obuf + T.at_cnt, T.cap, T.cap ? (float4*)(obuf + T.at_seg) : nullptr,
                        T.cap ? obuf + T.at_cell : nullptr);
    c->K.rev = rev;
    T.stage = 2u;
    return SPHX_OK;
}

int sphx_tile_contour_fetch(sphx_ctx* c, float* segments, uint32_t* cell, uint32_t* out_count) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_contour_fetch";
    if (!out_count) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out_count is NULL");
    *out_count = 0;
    if (!c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not a tile context");
    sphx_ctx::TileContour& T = c->tcontour;
    if (T.stage != 2u) return c->fail(SPHX_ERR_NOT_READY, fn, "no cut is waiting (sphx_tile_contour_cut first)");
    T.stage = 0u;
    if (!T.cells) return SPHX_OK;
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t* const obuf = (const uint32_t*)c->sample_buf;
    hipStream_t st = c->stream;
    uint32_t total = 0;
    SPHX_HIP(c, hipMemcpyAsync(&total, obuf + T.at_cnt, 4, hipMemcpyDeviceToHost, st));
    SPHX_HIP(c, hipStreamSynchronize(st));
    if (total > 2u * T.cells) return c->fail(SPHX_ERR_HIP, fn, "the tile counted more segments than two per cell");
    *out_count = total;
    const size_t got = std::min<size_t>(total, T.cap);
    if (got && segments) SPHX_HIP(c, hipMemcpyAsync(segments, obuf + T.at_seg, got * 16, hipMemcpyDeviceToHost, st));
    if (got && cell) SPHX_HIP(c, hipMemcpyAsync(cell, obuf + T.at_cell, got * 4, hipMemcpyDeviceToHost, st));
    if (got && (segments || cell)) SPHX_HIP(c, hipStreamSynchronize(st));
    return SPHX_OK;
}

}  // extern "C"
