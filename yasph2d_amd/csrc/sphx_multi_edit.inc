// sphx_multi_edit.inc — the device half of an edit of a tiled run (sphx_multi_append / sphx_multi_remove, include/sphx.h; the host half
// is in sphx_tiles.cpp, routing and the id counter in sphx_multi_edit.hpp): a tile retires the records it OWNS that a removal's predicate
// hits, and takes new owned records behind its local set.  The halo exchange and the re-grid that follow (TileDriver::refresh) do the rest:
// a retired record gets no cell, ghosts are rebuilt from what the owners pack.
// Included at the end of sphx_kernels.hip (one translation unit: the launch layer of sphx_launch.inc, EditRects / edit_removes /
// k_remove_scan of sphx_edit.inc and the tile checks of sphx_stats.inc are visible).

namespace sphx {

// One lane per local record, no atomics.  hit = owned (bit 31 of the id) and not retired before (x is not NaN) and the predicate removes
// the position.  A hit lane stores the retired mark into pos[i].x — the only write to the particle arrays; a lane that does not hit
// stores nothing.  Hits per wavefront by ballot, the four wavefronts meet in LDS, one word per workgroup leaves (k_remove_scan sums them).
// 12 bytes read per local record, 4 written per removed one, 4 per workgroup.
__global__ __launch_bounds__(256) void k_tile_remove_mark(const uint32_t* __restrict__ pid, float2* pos, uint32_t n, EditRects R, uint32_t* __restrict__ wg_hits) {
    __shared__ uint32_t wave_hits[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool hit = false;
    if (i < n) {
        const uint32_t id = pid[i];
        const float2 p = pos[i];
        hit = (id >> 31) != 0u && p.x == p.x && edit_removes(R, p);
    }
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & 63u) == 0u) wave_hits[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    if (hit) reinterpret_cast<uint32_t*>(pos + i)[0] = 0x7FC00000u;  // (i < n: inside the array)
    __syncthreads();
    if (threadIdx.x == 0u) wg_hits[blockIdx.x] = wave_hits[0] + wave_hits[1] + wave_hits[2] + wave_hits[3];
}

// The routed records from their staging copies into [from, from + m): owned, with fresh warm-start sums.  svel == nullptr: at rest.
__global__ __launch_bounds__(256) void k_tile_append(const float2* __restrict__ spos, const float2* __restrict__ svel, const uint32_t* __restrict__ sid, uint32_t m,
                                                       uint32_t from, float2* __restrict__ pos, float2* __restrict__ vel, uint32_t* __restrict__ pid,
                                                       float* __restrict__ kappa, float* __restrict__ stiff) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= m) return;
    const uint32_t d = from + k;  // (< from + m <= capN: the caller has grown the arrays)
    pos[d] = spos[k];
    vel[d] = svel ? svel[k] : make_float2(0.0f, 0.0f);
    pid[d] = sid[k] | 0x80000000u;
    kappa[d] = 0.0f;
    stiff[d] = 0.0f;
}

}  // namespace sphx

// ---- launch layer and the internal seam of the tile loop ---------------------------------------------------------------------------------
namespace {

// what edit_set_changed (sphx_edit.inc) voids, for a tile: the re-grid of the refresh that follows is the warm-up block, so no flag is kept
void tile_set_changed(sphx_ctx* c, const char* sample_message) {
    c->ahead.valid = false;
    drop_fused_count(c);  // (a cell count or a classification made for the old set is void)
    lists_went_stale(c);
    sample_went_stale(c, sample_message);
}

int tile_edit_scratch(sphx_ctx* c, size_t words) {
    if (words <= c->edit_cap) return SPHX_OK;
    if (words > 0xFFFFFFFFull) return c->fail(SPHX_ERR_CAPACITY, "the edit's scratch exceeds 2^32 words");
    SPHX_HIP(c, hipStreamSynchronize(c->stream));  // (a queued pass may still use the old buffer)
    c->edit_cap = 0;
    c->edit_mark = sphx_ctx::MARK_NONE;
    int rc;
    if ((rc = dev_alloc(c, &c->edit_buf, words))) return rc;
    c->edit_cap = (uint32_t)words;
    return SPHX_OK;
}

// room for `capacity` records.  The local set survives with everything that belongs to its particles in a tile: position, velocity, id and
// the two warm-start sums (alpha too; density is recomputed by the re-grid the caller runs next).
int tile_grow(sphx_ctx* c, uint32_t capacity) {
    if (capacity <= c->capN) return SPHX_OK;
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    tile_set_changed(c, "the tile's arrays were reallocated: run sphx_sub_regrid");
    c->cached_n = c->N;  // (alloc_particles keeps the slot-bound arrays of [0, cached_n): in a tile they are the particles' own)
    int rc;
    if ((rc = alloc_particles(c, capacity, edit_grown_capacity(c->capN, capacity), true))) return rc;
    // what sphx_tile_upload sizes by the capacity
    if ((rc = dev_alloc(c, &c->tile_blk, (size_t)(nblocks(c->capN) + 8) * MAX_TILE_PEERS + nblocks(c->capN) + 8))) return rc;
    const uint32_t need = nblocks(c->capN, std::min(SCAN_TILE, SCAN1_TILE)) + 1;
    if (need > c->scan_partials_cap) {
        if ((rc = dev_alloc(c, &c->scan_partials, need))) return rc;
        c->scan_partials_cap = need;
    }
    return ensure_index_scratch(c);
}

}  // namespace

extern "C" {

int sphx_tile_remove_mark(sphx_ctx* c, const sphx_rect* rects, uint32_t n_rects, uint32_t flags) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (n_rects > SPHX_REMOVE_MAX_RECTS) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_remove_mark: n_rects is larger than SPHX_REMOVE_MAX_RECTS");
    if (n_rects && !rects) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_remove_mark: rects is NULL with n_rects > 0");
    if (flags & ~(uint32_t)SPHX_REMOVE_OUTSIDE) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_remove_mark: unknown flags bits");
    sphx::EditRects R{};
    R.n = n_rects;
    R.outside = (flags & SPHX_REMOVE_OUTSIDE) ? 1u : 0u;
    for (uint32_t k = 0; k < n_rects; ++k) {
        R.r[k] = rects[k];
        if (std::isnan(rects[k].x0) || std::isnan(rects[k].y0) || std::isnan(rects[k].x1) || std::isnan(rects[k].y1))
            return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_remove_mark: a rectangle bound is NaN");
    }
    int rc;
    if ((rc = stats_check_tile(c, "sphx_tile_remove_mark"))) return rc;
    if ((rc = stats_check_tile_state(c, "sphx_tile_remove_mark"))) return rc;  // (the predicate needs the positions of the finished step)
    c->edit_mark = sphx_ctx::MARK_NONE;
    const uint32_t n = c->N;
    if (n == 0) {
        c->edit_mark = sphx_ctx::MARK_EMPTY;
        return SPHX_OK;
    }
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t nb = nblocks(n);
    if ((rc = tile_edit_scratch(c, (size_t)nb + 1u))) return rc;
    const uint32_t rev = c->K.rev;  // (an edit must not change the sweep direction of the step's next kernels: launch() toggles it)
    hipStream_t st = c->stream;
    uint32_t* const wg = c->edit_buf;
    launch(c, "tile_remove_mark", 12.0 * n + 4.0 * nb, [&] { hipLaunchKernelGGL(sphx::k_tile_remove_mark, dim3(nb), dim3(256), 0, st, (const uint32_t*)c->pid, c->posA, n, R, wg); });
    launch(c, "tile_remove_scan", 8.0 * nb + 4.0, [&] { hipLaunchKernelGGL(sphx::k_remove_scan, dim3(1), dim3(256), 0, st, wg, nb); });
    c->K.rev = rev;
    c->edit_mark = nb;
    return SPHX_OK;
}

int sphx_tile_remove_fetch(sphx_ctx* c, uint32_t* out_removed_owned) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (out_removed_owned) *out_removed_owned = 0;
    if (c->edit_mark == sphx_ctx::MARK_NONE) return c->fail(SPHX_ERR_NOT_READY, "sphx_tile_remove_fetch: no sphx_tile_remove_mark before it");
    const uint32_t nb = c->edit_mark;
    c->edit_mark = sphx_ctx::MARK_NONE;
    if (nb == sphx_ctx::MARK_EMPTY) return SPHX_OK;
    SPHX_HIP(c, hipSetDevice(c->device));
    uint32_t hits = 0;
    // the pass's only synchronisation: one word
    hipError_t e = hipMemcpyAsync(&hits, c->edit_buf + nb, 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess || hits > c->N) return c->fail(SPHX_ERR_HIP, "sphx_tile_remove_fetch: removed count", e != hipSuccess ? hipGetErrorString(e) : "larger than the local count");
    // nothing retired here: this context is as it was (lists, sampling state and a run-ahead pass stay valid)
    if (hits) tile_set_changed(c, "sphx_tile_remove_mark retired particles: run the halo exchange and sphx_sub_regrid");
    if (out_removed_owned) *out_removed_owned = hits;
    return SPHX_OK;
}

int sphx_tile_grow(sphx_ctx* c, uint32_t capacity) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = stats_check_tile(c, "sphx_tile_grow"))) return rc;
    if ((rc = stats_check_tile_state(c, "sphx_tile_grow"))) return rc;
    if (capacity >= (1u << 28)) return c->fail(SPHX_ERR_CAPACITY, "more than 2^28 fluid + boundary slots in one context: split the domain into more tiles");
    SPHX_HIP(c, hipSetDevice(c->device));
    return tile_grow(c, capacity);
}

int sphx_tile_append(sphx_ctx* c, const float* pos_xy, const float* vel_xy, const uint32_t* ids, uint32_t m) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (m && (!pos_xy || !ids)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_append: pos_xy or ids is NULL with n_new > 0");
    int rc;
    if ((rc = stats_check_tile(c, "sphx_tile_append"))) return rc;
    if (c->tile_pending_dt > 0.0f) return c->fail(SPHX_ERR_NOT_READY, "sphx_tile_append: the tile is between a halo exchange and its re-grid (sphx_sub_regrid first)");
    for (uint32_t k = 0; k < m; ++k) {
        if (!std::isfinite(pos_xy[2 * (size_t)k]) || !std::isfinite(pos_xy[2 * (size_t)k + 1]))
            return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_append: a position is not finite (a NaN x is the mark of a retired record)");
        if (ids[k] >> 31) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_append: an id is not below 2^31 (bit 31 is the owner bit)");
    }
    if (m == 0) return SPHX_OK;
    const uint32_t n = c->N;
    const uint64_t need = (uint64_t)n + m;
    if (need >= (1ull << 28)) return c->fail(SPHX_ERR_CAPACITY, "more than 2^28 fluid + boundary slots in one context: split the domain into more tiles");
    SPHX_HIP(c, hipSetDevice(c->device));
    if ((rc = tile_grow(c, (uint32_t)need))) return rc;
    if ((rc = tile_edit_scratch(c, 5ull * m))) return rc;
    hipStream_t st = c->stream;
    uint32_t* const stage = c->edit_buf;  // pos 2m | vel 2m | ids m
    float2* const spos = (float2*)stage;
    float2* const svel = (float2*)(stage + 2ull * m);
    uint32_t* const sid = stage + 4ull * m;
    SPHX_HIP(c, hipMemcpyAsync(spos, pos_xy, (size_t)m * 8, hipMemcpyHostToDevice, st));
    if (vel_xy) SPHX_HIP(c, hipMemcpyAsync(svel, vel_xy, (size_t)m * 8, hipMemcpyHostToDevice, st));
    SPHX_HIP(c, hipMemcpyAsync(sid, ids, (size_t)m * 4, hipMemcpyHostToDevice, st));
    const uint32_t rev = c->K.rev;
    launch(c, "tile_append", 20.0 * m + 28.0 * m, [&] {
        hipLaunchKernelGGL(sphx::k_tile_append, dim3(nblocks(m)), dim3(256), 0, st, (const float2*)spos, vel_xy ? (const float2*)svel : (const float2*)nullptr,
                           (const uint32_t*)sid, m, n, c->posA, c->vel, c->pid, c->kappa, c->stiff);
    });
    c->K.rev = rev;
    SPHX_HIP(c, hipStreamSynchronize(st));  // (the caller's arrays are borrowed for the duration of the call)
    c->N = (uint32_t)need;
    tile_set_changed(c, "sphx_tile_append added particles: run the halo exchange and sphx_sub_regrid");
    // the new particles' blocks join the dynamic directory (merged with the present coverage), as in sphx_append
    uint32_t bb[4];
    if (cell_bbox(c, pos_xy, m, bb)) {
        if (c->have_fluid_bbox) {
            c->fb[0] = std::min(c->fb[0], bb[0]);
            c->fb[1] = std::min(c->fb[1], bb[1]);
            c->fb[2] = std::max(c->fb[2], bb[2]);
            c->fb[3] = std::max(c->fb[3], bb[3]);
        } else {
            std::memcpy(c->fb, bb, sizeof(bb));
            c->have_fluid_bbox = true;
        }
    }
    if ((rc = cover_dynamic(c, pos_xy, m, false))) return rc;
    return ensure_index_scratch(c);
}

}  // extern "C"
