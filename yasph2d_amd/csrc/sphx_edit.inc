// sphx_edit.inc — fluid emitted into and drained from the device state between steps (sphx_append / sphx_remove, include/sphx.h): a small
// edit of the cell-ordered arrays instead of a download, a host-side filter or concatenation, and a fresh sphx_upload.
// Included at the end of sphx_kernels.hip (one translation unit: the launch layer of sphx_launch.inc is visible).

namespace sphx {

// the rectangles of one sphx_remove call, by value in the kernel arguments (136 bytes: scalar registers, no table in memory)
struct EditRects {
    sphx_rect r[SPHX_REMOVE_MAX_RECTS];
    uint32_t n;
    uint32_t outside;  // SPHX_REMOVE_OUTSIDE: the rectangles are a keep-box
};

// The predicate of sphx.h, in fp32 with IEEE comparisons: a NaN coordinate is in no rectangle (so it stays, or goes in OUTSIDE mode).
__device__ __forceinline__ bool edit_removes(const EditRects& R, float2 p) {
    bool hit = false;
#pragma unroll
    for (uint32_t k = 0; k < SPHX_REMOVE_MAX_RECTS; ++k)
        if (k < R.n) hit = hit || (p.x >= R.r[k].x0 && p.x < R.r[k].x1 && p.y >= R.r[k].y0 && p.y < R.r[k].y1);
    return R.outside ? !hit : hit;
}

// Stable compaction in three launches (DESIGN.md §4e).  Workgroups are taken in blockIdx.x order — not xcd_bid(): workgroup b's survivors
// go behind those of the workgroups 0 .. b - 1, whichever XCD ran them.  No atomic decides a slot.
// pass 1: survivors per workgroup of 256 particles
__global__ __launch_bounds__(256) void k_remove_flag(const float2* __restrict__ pos, uint32_t n, EditRects R, uint32_t* __restrict__ wg_kept) {
    __shared__ uint32_t wave_kept[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool keep = i < n && !edit_removes(R, pos[i]);
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63u) == 0u) wave_kept[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0u) wg_kept[blockIdx.x] = wave_kept[0] + wave_kept[1] + wave_kept[2] + wave_kept[3];
}

// pass 2, one workgroup: wg[0 .. nb) becomes its exclusive prefix sum, wg[nb] the total (the one word the host reads back).  Lane t owns
// the contiguous piece [t * per, (t + 1) * per): at 16 M particles 256 words per lane out of a 256 KiB array.
__global__ __launch_bounds__(256) void k_remove_scan(uint32_t* __restrict__ wg, uint32_t nb) {
    __shared__ uint32_t piece[256];
    const uint32_t per = (nb + 255u) / 256u;
    const uint32_t b0 = min(threadIdx.x * per, nb), b1 = min(b0 + per, nb);
    uint32_t s = 0;
    for (uint32_t b = b0; b < b1; ++b) s += wg[b];
    piece[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < 256u; ++k) {
            const uint32_t t = piece[k];
            piece[k] = run;
            run += t;
        }
        wg[nb] = run;
    }
    __syncthreads();
    uint32_t run = piece[threadIdx.x];
    for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t t = wg[b];
        wg[b] = run;
        run += t;
    }
}

// pass 3: the survivors' records to their slots.  Slot = workgroup offset + survivors of the wavefronts before this one (LDS) + rank among
// the wavefront's survivors (ballot + mbcnt).  Position, velocity and id travel (8-, 8- and 4-byte accesses); everything else is slot-bound.
__global__ __launch_bounds__(256) void k_remove_move(const float2* __restrict__ pos, const float2* __restrict__ vel, const uint32_t* __restrict__ pid,
                                                     uint32_t n, EditRects R, const uint32_t* __restrict__ wg_off, float2* __restrict__ pos2,
                                                     float2* __restrict__ vel2, uint32_t* __restrict__ pid2) {
    __shared__ uint32_t wave_kept[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const float2 p = i < n ? pos[i] : make_float2(0.0f, 0.0f);
    const bool keep = i < n && !edit_removes(R, p);
    const unsigned long long m = __ballot(keep);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) wave_kept[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t base = wg_off[blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) base += k < w ? wave_kept[k] : 0u;
    if (keep) {
        const uint32_t d = base + rank;  // (< the survivor total <= n: inside the arrays)
        pos2[d] = p;
        vel2[d] = vel[i];
        pid2[d] = pid[i];
    }
}

// sphx_append: ids of the new records [from, from + m)
__global__ __launch_bounds__(256) void k_append_ids(uint32_t* __restrict__ pid, uint32_t from, uint32_t m, uint32_t first_id) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < m) pid[from + k] = first_id + k;
}

}  // namespace sphx

// ---- launch layer and C ABI ----------------------------------------------------------------------------------------------------------
namespace {

// capacity growth of sphx_append: half as much again (an emitter that adds a block every few steps reallocates O(log) times)
inline uint32_t edit_grown_capacity(uint32_t cap_now, uint64_t need) {
    const uint64_t grown = (uint64_t)cap_now + cap_now / 2u;
    return (uint32_t)std::min<uint64_t>(std::max(grown, need), 0xFFFFFFFFull);
}

// the refusals both calls share
int edit_check_state(sphx_ctx* c, const char* fn) {
    const std::string f = fn;
    if (c->tile_mode)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": not available on a tile context (its arrays hold ghosts and miss the particles other tiles own)").c_str());
    if (c->tiling_invariant)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": not available in tiling-invariant mode (its warm-start values travel with the particles)").c_str());
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, (f + ": between step_begin and step_finish (finish the step first)").c_str());
    if (!c->uploaded) return c->fail(SPHX_ERR_NOT_READY, (f + ": no particles uploaded (an upload of zero particles is enough)").c_str());
    return SPHX_OK;
}

// the particle set is another one now: what every call that changed it leaves behind
void edit_set_changed(sphx_ctx* c, const char* sample_message) {
    c->set_changed = true;  // the next sphx_step_begin runs the warm-up block, whatever the count
    c->ahead.valid = false;
    drop_fused_count(c);  // (a cell count made for the old set is void; the histograms stay all-zero)
    lists_went_stale(c);
    sample_went_stale(c, sample_message);
}

}  // namespace

extern "C" {

int sphx_remove(sphx_ctx* c, const sphx_rect* rects, uint32_t n_rects, uint32_t flags, uint32_t* out_removed) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (out_removed) *out_removed = 0;
    if (n_rects > SPHX_REMOVE_MAX_RECTS) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_remove: n_rects is larger than SPHX_REMOVE_MAX_RECTS");
    if (n_rects && !rects) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_remove: rects is NULL with n_rects > 0");
    if (flags & ~(uint32_t)SPHX_REMOVE_OUTSIDE) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_remove: unknown flags bits");
    EditRects R{};
    R.n = n_rects;
    R.outside = (flags & SPHX_REMOVE_OUTSIDE) ? 1u : 0u;
    for (uint32_t k = 0; k < n_rects; ++k) {
        R.r[k] = rects[k];
        if (std::isnan(rects[k].x0) || std::isnan(rects[k].y0) || std::isnan(rects[k].x1) || std::isnan(rects[k].y1))
            return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_remove: a rectangle bound is NaN");
    }
    int rc;
    if ((rc = edit_check_state(c, "sphx_remove"))) return rc;
    const uint32_t n = c->N;
    if (n == 0) return SPHX_OK;
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t nb = (n + 255u) / 256u;
    if (nb + 1u > c->edit_cap) {
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
        if ((rc = dev_alloc(c, &c->edit_buf, (size_t)nb + 1u))) {
            c->edit_cap = 0;
            return rc;
        }
        c->edit_cap = nb + 1u;
    }
    const uint32_t rev = c->K.rev;  // (an edit must not change the sweep direction of the step's next kernels: launch() toggles it)
    hipStream_t st = c->stream;
    uint32_t* const wg = c->edit_buf;
    launch(c, "remove_flag", 8.0 * n + 4.0 * nb,
           [&] { hipLaunchKernelGGL(k_remove_flag, dim3(nb), dim3(256), 0, st, (const float2*)c->posA, n, R, wg); });
    launch(c, "remove_scan", 8.0 * nb + 4.0, [&] { hipLaunchKernelGGL(k_remove_scan, dim3(1), dim3(256), 0, st, wg, nb); });
    uint32_t kept = 0;
    // the call's only synchronisation: one word
    hipError_t e = hipMemcpyAsync(&kept, wg + nb, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess || kept > n) {
        c->K.rev = rev;
        return c->fail(SPHX_ERR_HIP, "sphx_remove: survivor count", e != hipSuccess ? hipGetErrorString(e) : "larger than the particle count");
    }
    const uint32_t removed = n - kept;
    if (removed == 0) {  // nothing removed: the context is as it was (lists, sampling state and a run-ahead pass stay valid)
        c->K.rev = rev;
        return SPHX_OK;
    }
    if (kept) {
        launch(c, "remove_move", 8.0 * n + 4.0 * nb + 40.0 * kept, [&] {
            hipLaunchKernelGGL(k_remove_move, dim3(nb), dim3(256), 0, st, (const float2*)c->posA, (const float2*)c->vel, (const uint32_t*)c->pid, n, R,
                               (const uint32_t*)wg, c->posA2, c->vel2, c->pid2);
        });
        // (the boundary tails at soff() exist in both array pairs: nothing to do for them)
        std::swap(c->posA, c->posA2);
        std::swap(c->vel, c->vel2);
        std::swap(c->pid, c->pid2);
    }
    c->K.rev = rev;
    c->N = kept;
    edit_set_changed(c, "sphx_remove changed the particle set: run a step, or sphx_update_neighborhood + sphx_update_densities");
    if (out_removed) *out_removed = removed;
    return SPHX_OK;
}

int sphx_append(sphx_ctx* c, const float* pos_xy, const float* vel_xy, uint32_t m, uint32_t* out_first_id) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (m && !pos_xy) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_append: pos_xy is NULL with m > 0");
    int rc;
    if ((rc = edit_check_state(c, "sphx_append"))) return rc;
    if (c->ids_issued + m > (1ull << 32)) return c->fail(SPHX_ERR_CAPACITY, "sphx_append: more than 2^32 particle ids since the last sphx_upload (ids are never reused)");
    const uint32_t first_id = (uint32_t)c->ids_issued;  // (== 2^32 only with m == 0: nothing is numbered then)
    if (out_first_id) *out_first_id = first_id;
    if (m == 0) return SPHX_OK;
    const uint32_t n = c->N;
    const uint64_t need = (uint64_t)n + m;
    if (need >= (1ull << 28)) return c->fail(SPHX_ERR_CAPACITY, "more than 2^28 fluid + boundary slots in one context: split the domain into tiles");
    SPHX_HIP(c, hipSetDevice(c->device));
    if (need > c->capN) {
        // geometric growth; positions, velocities and ids of [0, n) are copied over, the slot-bound arrays kept as sphx_upload keeps them
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
        if ((rc = alloc_particles(c, (uint32_t)need, edit_grown_capacity(c->capN, need), true))) return rc;
    }
    hipStream_t st = c->stream;
    SPHX_HIP(c, hipMemcpyAsync(c->posA + n, pos_xy, (size_t)m * 8, hipMemcpyHostToDevice, st));
    if (vel_xy)
        SPHX_HIP(c, hipMemcpyAsync(c->vel + n, vel_xy, (size_t)m * 8, hipMemcpyHostToDevice, st));
    else
        SPHX_HIP(c, hipMemsetAsync(c->vel + n, 0, (size_t)m * 8, st));
    const uint32_t rev = c->K.rev;
    launch(c, "append", 4.0 * m, [&] { hipLaunchKernelGGL(k_append_ids, dim3((m + 255u) / 256u), dim3(256), 0, st, c->pid, n, m, first_id); });
    c->K.rev = rev;
    SPHX_HIP(c, hipStreamSynchronize(st));  // (the caller's arrays are borrowed for the duration of the call)
    c->N = (uint32_t)need;
    c->ids_issued += m;
    edit_set_changed(c, "sphx_append changed the particle set: run a step, or sphx_update_neighborhood + sphx_update_densities");
    // the new particles' blocks join the dynamic directory (merged with the present coverage), and the upload's cell bounding box widens
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
