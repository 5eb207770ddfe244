// sphx_query.inc — the cell grids as a search service: which particles lie around given points (sphx_query_radius) and which lie in
// given rectangles (sphx_select); the contract is in include/sphx.h, "neighbour queries", restated bit for bit by tests/query_reference.py.
// Included at the end of sphx_kernels.hip behind sphx_contour.inc (one translation unit: cell_of, slots9n, ranges9n, gat,
// block_excl_scan_256, EditRects / k_remove_flag / k_remove_scan of sphx_edit.inc and the launch layer are visible).
// sphx_query_radius, one lane per point, 256 points per workgroup:
//   k_query_count    walks the 3 x 3 box of its point, stores the point's exclusive prefix inside the workgroup, the nearest accepted
//                    candidate, and the workgroup's total;
//   k_query_carry    one workgroup turns the totals into 64-bit exclusive offsets, chunk after chunk in ascending order (the scheme of
//                    k_contour_carry), and stores the grand total;
//   k_query_emit     walks again; entry `rank` of its point goes to offset-of-workgroup + prefix-in-workgroup + rank, through an LDS
//                    stage that lets the workgroup store whole lines (k_query_offsets finishes offsets[] where no list is wanted).
// sphx_select: sphx_remove's flag and scan passes with the predicate inverted, then k_select_emit.
// One tile of a tiled run (sphx_tile_query_radius / sphx_tile_select, "neighbour queries of a tiled run"): the tile answers the points
// whose cell it owns.  k_query_own_flag / k_remove_scan / k_query_own_list put their indices into list[] in ascending point index (a stable
// compaction: the list, and with it the layout of the tile's entries, is the same in every call — k_tile_sample_select's atomic would make
// it differ); k_query_count / k_query_emit then run in their LIST form, lane k serving point list[k], every lane of every full workgroup
// live.  sphx_tile_select: k_tile_select_flag / k_remove_scan / k_tile_select_emit, the predicate with "owned" (bit 31 of the id) added.
// No atomic anywhere: every position is fixed by the point (particle) order.  Compiled with -ffp-contract=off like the rest.

namespace sphx {

// the set one call answers over: the fluid (pos = posA, off = 0, ids = particle_id) or the boundary (off = soff, ids = boundary_id)
struct QueryArgs {
    const float2* pos;
    uint32_t off;
    const uint32_t* ids;
    NbGrid g;
    float r2;
    uint32_t empty;  // the set holds nothing (no grid to walk): every point gets an empty list
};
constexpr uint32_t QUERY_MAX_BLOCKS = 1u << 22;  // workgroups per launch, as SAMPLE_MAX_BLOCKS

// exclusive scan over the 256 threads of a block for values below 2^(16 LIMBS), exact in 64 bits: one block_excl_scan_256 per 16-bit
// limb (256 limbs sum to less than 2^24)
template <int LIMBS>
__device__ __forceinline__ unsigned long long query_scan_256(unsigned long long v, unsigned long long* total) {
    unsigned long long ex = 0, tot = 0;
#pragma unroll
    for (int l = 0; l < LIMBS; ++l) {
        uint32_t t;
        const uint32_t e = block_excl_scan_256((uint32_t)(v >> (16 * l)) & 0xFFFFu, &t);
        ex += (unsigned long long)e << (16 * l);
        tot += (unsigned long long)t << (16 * l);
    }
    *total = tot;
    return ex;
}

// The walk of ONE query point: sample_walk's candidates of one set, accept(j, d2) per accepted candidate in candidate order.  A dead
// lane (live = false) takes part in the wavefront's directory look-ups and walks nothing.
template <class F>
__device__ __forceinline__ void query_walk(const Consts& K, const QueryArgs& a, float qx, float qy, bool live, F&& accept) {
    if (a.empty) return;  // (uniform over the launch)
    uint32_t cx, cy;
    cell_of(K, make_float2(qx, qy), cx, cy);  // a NaN coordinate saturates to cell 0, and every distance test with it fails
    uint32_t slot[9], s[9], e[9], centre, any9;
    slots9n(a.g, cx, cy, slot, centre, any9);
    ranges9n(a.g, slot, s, e);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const uint32_t end = live ? e[t] : s[t];
        for (uint32_t j = s[t]; j < end; ++j) {
            const float2 pj = gat(a.pos, a.off + j);
            const float dx = pj.x - qx, dy = pj.y - qy;
            const float d2 = dx * dx + dy * dy;
            if (d2 <= a.r2) accept(j, d2);
        }
    }
}

// The LIST form of the two walks (one tile of a tiled run): record i of the launch is point list[i], n[0] records in all — a device word,
// the launch is sized for all m points and a workgroup behind the list leaves at once (no host round trip between the selection and the
// walk).  Ids lose the owner bit (id_mask), the nearest candidate's id is stored next to its index.  The plain form carries an empty
// struct: the single context's kernels keep their arguments and their code.
template <bool LIST>
struct QueryList {};
template <>
struct QueryList<true> {
    const uint32_t* list;  // [n[0]] ascending point indices
    const uint32_t* n;     // [1]
    uint32_t* nearest_id;  // [n[0]] or null
    uint32_t id_mask;
};

// pass 1: workgroup base + blockIdx.x owns the points [256 b, 256 b + 256) of xy[] (caller order).  pref[i] = accepted candidates of the
// workgroup's points before i; wg_total[b] = those of the whole workgroup.
template <bool NEAREST, bool LIST>
__global__ __launch_bounds__(256) void k_query_count(Consts K, QueryArgs a, const float* __restrict__ xy, uint32_t m, uint32_t base,
                                                     unsigned long long* __restrict__ pref, unsigned long long* __restrict__ wg_total,
                                                     uint32_t* __restrict__ nearest, float* __restrict__ nearest_d2, QueryList<LIST> L) {
    const uint32_t b = base + blockIdx.x, i = b * 256u + threadIdx.x;
    if constexpr (LIST) {
        m = L.n[0];
        if (b * 256u >= m) {  // (workgroup-uniform: behind the list — the carry still reads this workgroup's total)
            if (threadIdx.x == 0) wg_total[b] = 0ull;
            return;
        }
    }
    const bool live = i < m;
    uint32_t k = live ? i : m - 1u;  // (m > 0: the host launches nothing for an empty set)
    if constexpr (LIST) k = L.list[k];
    uint32_t cnt = 0, best = SPHX_QUERY_NONE;
    float best_d2 = __uint_as_float(0x7F800000u);
    query_walk(K, a, xy[2 * (size_t)k], xy[2 * (size_t)k + 1], live, [&](uint32_t j, float d2) {
        cnt += 1u;
        if (NEAREST && d2 < best_d2) {  // (candidate order: a tie keeps the lower index)
            best_d2 = d2;
            best = j;
        }
    });
    unsigned long long total;
    const unsigned long long ex = query_scan_256<2>(cnt, &total);
    if (live) {
        pref[i] = ex;
        if (NEAREST && nearest) nearest[i] = best;
        if (NEAREST && nearest_d2) nearest_d2[i] = best_d2;
        if constexpr (LIST) {
            if (NEAREST && L.nearest_id) L.nearest_id[i] = best == SPHX_QUERY_NONE ? SPHX_QUERY_NONE : (gat(a.ids, best) & L.id_mask);
        }
    }
    if (threadIdx.x == 0) wg_total[b] = total;
}

// across workgroups: ONE workgroup walks the totals in chunks of 256 in ascending order and replaces each by the sum of all before it;
// the grand total goes to *count and behind the points' offsets.  (A workgroup's total is below 256 * 2^28: three limbs.)
__global__ __launch_bounds__(256) void k_query_carry(unsigned long long* __restrict__ wg, uint32_t nblocks, unsigned long long* __restrict__ count,
                                                     unsigned long long* __restrict__ off_end) {
    unsigned long long carry = 0;
    for (uint32_t i0 = 0; i0 < nblocks; i0 += 256u) {  // (workgroup-uniform bounds)
        const uint32_t i = i0 + threadIdx.x;
        const unsigned long long v = i < nblocks ? wg[i] : 0ull;
        unsigned long long total;
        const unsigned long long ex = query_scan_256<3>(v, &total);
        if (i < nblocks) wg[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        count[0] = carry;
        if (off_end) off_end[0] = carry;
    }
}

// offsets[i] = offset of the workgroup + prefix inside it, where no list is wanted (k_query_emit does it otherwise)
__global__ __launch_bounds__(256) void k_query_offsets(unsigned long long* __restrict__ pref, const unsigned long long* __restrict__ wg, uint32_t m,
                                                       uint32_t base) {
    const uint32_t b = base + blockIdx.x, i = b * 256u + threadIdx.x;
    if (i < m) pref[i] += wg[b];
}

// pass 2: the walk again; entry `rank` of point i goes to wg[b] + pref[i] + rank if that is below the capacity.  The entries of a
// workgroup are contiguous, [wg[b], wg[b + 1]).  Up to QUERY_STAGE of them are staged in LDS at pref[i] + rank (index and d2, 8 bytes)
// and stored by the whole workgroup, lane after lane in whole lines, the ids gathered on the way out: a lane storing its own run makes
// every store instruction of a wavefront touch 64 runs (DESIGN.md section 4r).  A workgroup with more (a dense neighbourhood) stores directly.
constexpr uint32_t QUERY_STAGE = 4096;  // 32 KiB
template <bool LIST>
__global__ __launch_bounds__(256) void k_query_emit(Consts K, QueryArgs a, const float* __restrict__ xy, uint32_t m, uint32_t base, uint32_t nblocks,
                                                    unsigned long long* __restrict__ pref, const unsigned long long* __restrict__ wg,
                                                    const unsigned long long* __restrict__ count, uint32_t keep_offsets, unsigned long long cap,
                                                    uint32_t* __restrict__ index, uint32_t* __restrict__ id, float* __restrict__ dist_sq, QueryList<LIST> L) {
    __shared__ uint2 stage[QUERY_STAGE];
    const uint32_t b = base + blockIdx.x, i = b * 256u + threadIdx.x;
    if constexpr (LIST) {
        m = L.n[0];
        if (b * 256u >= m) return;  // (workgroup-uniform: behind the list)
    }
    const bool live = i < m;
    uint32_t k = live ? i : m - 1u;
    if constexpr (LIST) k = L.list[k];
    const unsigned long long first = wg[b];
    const unsigned long long total = (b + 1u < nblocks ? wg[b + 1u] : count[0]) - first;  // (workgroup-uniform)
    unsigned long long local = 0;
    if (live) {
        local = pref[i];
        if (keep_offsets) pref[i] = first + local;
    }
    const float qx = xy[2 * (size_t)k], qy = xy[2 * (size_t)k + 1];
    if (total <= QUERY_STAGE) {
        uint32_t at = (uint32_t)local;
        query_walk(K, a, qx, qy, live && first + local < cap, [&](uint32_t j, float d2) {
            if (at < QUERY_STAGE) stage[at] = make_uint2(j, __float_as_uint(d2));  // (always: pass 1 counted these very entries)
            at += 1u;
        });
        __syncthreads();
        const uint32_t n = first < cap ? (uint32_t)min(total, cap - first) : 0u;
        for (uint32_t e = threadIdx.x; e < n; e += 256u) {
            const uint2 r = stage[e];
            if (index) index[first + e] = r.x;
            if constexpr (LIST) {
                if (id) id[first + e] = gat(a.ids, r.x) & L.id_mask;
            } else {
                if (id) id[first + e] = gat(a.ids, r.x);
            }
            if (dist_sq) dist_sq[first + e] = __uint_as_float(r.y);
        }
        return;
    }
    unsigned long long at = first + local;
    query_walk(K, a, qx, qy, live && at < cap, [&](uint32_t j, float d2) {
        if (at < cap) {
            if (index) index[at] = j;
            if constexpr (LIST) {
                if (id) id[at] = gat(a.ids, j) & L.id_mask;
            } else {
                if (id) id[at] = gat(a.ids, j);
            }
            if (dist_sq) dist_sq[at] = d2;
        }
        at += 1ull;
    });
}

// sphx_select, pass 3: k_remove_move's slots, with the index and the id of a selected particle stored below the capacity instead of its
// record.  R is the call's predicate INVERTED (outside toggled), so that "kept" by sphx_remove's passes means selected.
__global__ __launch_bounds__(256) void k_select_emit(const float2* __restrict__ pos, const uint32_t* __restrict__ pid, uint32_t n, EditRects R,
                                                     const uint32_t* __restrict__ wg_off, uint32_t cap, uint32_t* __restrict__ index,
                                                     uint32_t* __restrict__ id) {
    __shared__ uint32_t wave_kept[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const float2 p = i < n ? pos[i] : make_float2(0.0f, 0.0f);
    const bool keep = i < n && !edit_removes(R, p);
    const unsigned long long m = __ballot(keep);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) wave_kept[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t d = wg_off[blockIdx.x] + rank;
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) d += k < w ? wave_kept[k] : 0u;
    if (keep && d < cap) {
        if (index) index[d] = i;
        if (id) id[d] = pid[i];
    }
}

// ---- one tile of a tiled run ------------------------------------------------------------------------------------------------------------
// the points this tile answers: those whose cell lies in its owned rectangle.  Pass 1: their number per workgroup of 256 points (ballot +
// population count per wavefront, the four meet in LDS); k_remove_scan turns the workgroups' numbers into exclusive offsets and the total.
__device__ __forceinline__ bool query_owns(const Consts& K, const float2* __restrict__ xy, uint32_t i, uint32_t m) {
    if (i >= m) return false;
    uint32_t cx, cy;
    cell_of(K, xy[i], cx, cy);  // (a NaN coordinate goes to cell 0: the tile that owns cell 0 answers it, with an empty list)
    return rect_has(K.tile, cx, cy, 0u);
}
__global__ __launch_bounds__(256) void k_query_own_flag(Consts K, const float2* __restrict__ xy, uint32_t m, uint32_t* __restrict__ wg_own) {
    __shared__ uint32_t wave_own[4];
    const bool own = query_owns(K, xy, blockIdx.x * 256u + threadIdx.x, m);
    const unsigned long long b = __ballot(own);
    if ((threadIdx.x & 63u) == 0u) wave_own[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0u) wg_own[blockIdx.x] = wave_own[0] + wave_own[1] + wave_own[2] + wave_own[3];
}
// pass 3: list[offset of the workgroup + owned points of the wavefronts before this one + rank in the wavefront] = i: ascending point index
__global__ __launch_bounds__(256) void k_query_own_list(Consts K, const float2* __restrict__ xy, uint32_t m, const uint32_t* __restrict__ wg_off,
                                                        uint32_t* __restrict__ list) {
    __shared__ uint32_t wave_own[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool own = query_owns(K, xy, i, m);
    const unsigned long long b = __ballot(own);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) wave_own[w] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t d = wg_off[blockIdx.x] + rank;
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) d += k < w ? wave_own[k] : 0u;
    if (own) list[d] = i;  // (d < the owned total <= m: inside the list)
}

// sphx_tile_select: k_remove_flag and k_select_emit with "owned by this tile" (bit 31 of the id word) added to the predicate; the id
// leaves with the bit cleared.  R is the call's predicate INVERTED, as in sphx_select.
__global__ __launch_bounds__(256) void k_tile_select_flag(const float2* __restrict__ pos, const uint32_t* __restrict__ pid, uint32_t n, EditRects R,
                                                          uint32_t* __restrict__ wg_kept) {
    __shared__ uint32_t wave_kept[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool keep = i < n && (pid[i] >> 31) != 0u && !edit_removes(R, pos[i]);
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63u) == 0u) wave_kept[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0u) wg_kept[blockIdx.x] = wave_kept[0] + wave_kept[1] + wave_kept[2] + wave_kept[3];
}
__global__ __launch_bounds__(256) void k_tile_select_emit(const float2* __restrict__ pos, const uint32_t* __restrict__ pid, uint32_t n, EditRects R,
                                                          const uint32_t* __restrict__ wg_off, uint32_t cap, uint32_t* __restrict__ index,
                                                          uint32_t* __restrict__ id) {
    __shared__ uint32_t wave_kept[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t word = i < n ? pid[i] : 0u;
    const bool keep = i < n && (word >> 31) != 0u && !edit_removes(R, pos[i]);
    const unsigned long long m = __ballot(keep);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) wave_kept[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t d = wg_off[blockIdx.x] + rank;
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) d += k < w ? wave_kept[k] : 0u;
    if (keep && d < cap) {
        index[d] = i;
        id[d] = word & 0x7FFFFFFFu;
    }
}

}  // namespace sphx

// ---- launch layer and C ABI ----------------------------------------------------------------------------------------------------------
namespace {

// a scratch of the two calls in 4-byte words, grown on demand (the stream is drained before the old one is freed)
int query_scratch(sphx_ctx* c, uint32_t** buf, size_t* cap, size_t words) {
    if (words <= *cap && *buf) return SPHX_OK;
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    int rc;
    if ((rc = dev_alloc(c, buf, words))) {
        *cap = 0;
        return rc;
    }
    *cap = words;
    return SPHX_OK;
}

template <class F>
void query_pieces(uint32_t nblocks, F&& f) {
    for (uint32_t b0 = 0; b0 < nblocks; b0 += sphx::QUERY_MAX_BLOCKS) f(std::min(nblocks - b0, sphx::QUERY_MAX_BLOCKS), b0);
}

// pass 1 and the carry on the context's stream
void query_enqueue_count(sphx_ctx* c, const sphx::QueryArgs& a, const float* d_xy, uint32_t m, unsigned long long* d_pref, unsigned long long* d_wg,
                         unsigned long long* d_cnt, bool offsets_end, uint32_t* d_near, float* d_near_d2, const sphx::QueryList<true>* list = nullptr) {
    hipStream_t st = c->stream;
    const uint32_t nblocks = (uint32_t)(((uint64_t)m + 255u) / 256u);
    // algorithmic bytes per point: the point, its prefix, ~ (9 cells) x (8-byte table entry) + the candidates' positions
    const double per = 8.0 + 8.0 + 72.0 + (d_near ? 4.0 : 0.0) + (d_near_d2 ? 4.0 : 0.0);
    query_pieces(nblocks, [&](uint32_t nb, uint32_t b0) {
        launch(c, "query_count", per * 256.0 * nb, [&] {
            const sphx::QueryList<false> plain{};
            if (list && (d_near || d_near_d2 || list->nearest_id))
                hipLaunchKernelGGL((sphx::k_query_count<true, true>), dim3(nb), dim3(256), 0, st, c->K, a, d_xy, m, b0, d_pref, d_wg, d_near, d_near_d2, *list);
            else if (list)
                hipLaunchKernelGGL((sphx::k_query_count<false, true>), dim3(nb), dim3(256), 0, st, c->K, a, d_xy, m, b0, d_pref, d_wg, d_near, d_near_d2, *list);
            else if (d_near || d_near_d2)
                hipLaunchKernelGGL((sphx::k_query_count<true, false>), dim3(nb), dim3(256), 0, st, c->K, a, d_xy, m, b0, d_pref, d_wg, d_near, d_near_d2, plain);
            else
                hipLaunchKernelGGL((sphx::k_query_count<false, false>), dim3(nb), dim3(256), 0, st, c->K, a, d_xy, m, b0, d_pref, d_wg, d_near, d_near_d2, plain);
        });
    });
    launch(c, "query_carry", 16.0 * nblocks, [&] {
        hipLaunchKernelGGL(sphx::k_query_carry, dim3(1), dim3(256), 0, st, d_wg, nblocks, d_cnt, offsets_end ? d_pref + m : (unsigned long long*)nullptr);
    }, false);
}
// offsets[] alone
void query_enqueue_offsets(sphx_ctx* c, uint32_t m, unsigned long long* d_pref, const unsigned long long* d_wg) {
    hipStream_t st = c->stream;
    query_pieces((uint32_t)(((uint64_t)m + 255u) / 256u), [&](uint32_t nb, uint32_t b0) {
        launch(c, "query_offsets", 16.0 * 256.0 * nb, [&] { hipLaunchKernelGGL(sphx::k_query_offsets, dim3(nb), dim3(256), 0, st, d_pref, d_wg, m, b0); }, false);
    });
}
// pass 2 (and offsets[] with it)
void query_enqueue_emit(sphx_ctx* c, const sphx::QueryArgs& a, const float* d_xy, uint32_t m, unsigned long long* d_pref, const unsigned long long* d_wg,
                        const unsigned long long* d_cnt, bool keep_offsets, uint64_t cap, uint32_t* d_index, uint32_t* d_id, float* d_d2,
                        const sphx::QueryList<true>* list = nullptr) {
    hipStream_t st = c->stream;
    const uint32_t nblocks = (uint32_t)(((uint64_t)m + 255u) / 256u);
    query_pieces(nblocks, [&](uint32_t nb, uint32_t b0) {
        launch(c, "query_emit", (8.0 + 16.0 + 72.0) * 256.0 * nb, [&] {
            if (list)
                hipLaunchKernelGGL(sphx::k_query_emit<true>, dim3(nb), dim3(256), 0, st, c->K, a, d_xy, m, b0, nblocks, d_pref, d_wg, d_cnt, keep_offsets ? 1u : 0u,
                                   (unsigned long long)cap, d_index, d_id, d_d2, *list);
            else
                hipLaunchKernelGGL(sphx::k_query_emit<false>, dim3(nb), dim3(256), 0, st, c->K, a, d_xy, m, b0, nblocks, d_pref, d_wg, d_cnt, keep_offsets ? 1u : 0u,
                                   (unsigned long long)cap, d_index, d_id, d_d2, sphx::QueryList<false>{});
        });
    });
}

}  // namespace

extern "C" {

int sphx_query_radius(sphx_ctx* c, const float* xy, uint32_t m, float radius, uint64_t cap_entries, uint32_t flags, const sphx_query_out* out) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_query_radius";
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out is NULL");
    if (!out->count) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out->count is NULL");
    if (m && !xy) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "xy is NULL with m > 0");
    if (flags & ~(uint32_t)(SPHX_QUERY_DEVICE_POINTERS | SPHX_QUERY_BOUNDARY)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "unknown flags bits");
    if (m >= (1u << 31)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "m must be < 2^31");
    if (!std::isfinite(radius) || !(radius > 0.0f) || radius > c->P.smoothing_length)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "radius must be finite, > 0 and <= smoothing_length");
    const bool device = (flags & SPHX_QUERY_DEVICE_POINTERS) != 0u, boundary = (flags & SPHX_QUERY_BOUNDARY) != 0u;
    if (device && ((uintptr_t)out->count & 7u)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out->count must be 8-byte aligned (a 64-bit word)");
    if (device && ((uintptr_t)out->offsets & 7u)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out->offsets must be 8-byte aligned (64-bit words)");
    if (c->tile_mode)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not available on a tile context (its arrays hold ghosts and miss the particles other tiles own)");
    if (m == 0) {  // (as sphx_sample_points: an empty set is answered once the arguments pass)
        if (!device) {
            out->count[0] = 0u;
            if (out->offsets) out->offsets[0] = 0u;
            return SPHX_OK;
        }
        SPHX_HIP(c, hipSetDevice(c->device));
        SPHX_HIP(c, hipMemsetAsync(out->count, 0, 8, c->stream));
        if (out->offsets) SPHX_HIP(c, hipMemsetAsync(out->offsets, 0, 8, c->stream));
        return SPHX_OK;
    }
    int rc;
    if ((rc = sample_check_state(c, fn))) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));

    sphx::QueryArgs a{};
    a.pos = (const float2*)c->posA;
    a.off = boundary ? c->soff() : 0u;
    a.ids = boundary ? (const uint32_t*)c->bid : (const uint32_t*)c->pid;
    const Grid& g = boundary ? c->gstat : c->gdyn;
    a.g = g.nview();
    a.r2 = radius * radius;
    a.empty = ((boundary ? c->B : c->N) == 0u || !g.dirn || !g.fine) ? 1u : 0u;

    const uint32_t nblocks = (uint32_t)(((uint64_t)m + 255u) / 256u);
    const bool lists = out->index || out->id || out->dist_sq;
    hipStream_t st = c->stream;
    const uint32_t rev = c->K.rev;  // (launch() toggles the sweep direction of the step's next kernels: put back below)
    if (device) {
        // scratch (64-bit words): workgroup offsets [nblocks] | prefixes [m + 1] unless the caller's offsets[] takes them
        const bool walk2 = lists && cap_entries > 0u;
        if ((rc = query_scratch(c, &c->query_buf, &c->query_cap, 2 * ((size_t)nblocks + (out->offsets ? 0 : (size_t)m + 1u))))) return rc;
        unsigned long long* const d_wg = (unsigned long long*)c->query_buf;
        unsigned long long* const d_pref = out->offsets ? (unsigned long long*)out->offsets : d_wg + nblocks;
        query_enqueue_count(c, a, xy, m, d_pref, d_wg, (unsigned long long*)out->count, out->offsets != nullptr, out->nearest, out->nearest_dist_sq);
        if (walk2) query_enqueue_emit(c, a, xy, m, d_pref, d_wg, (const unsigned long long*)out->count, out->offsets != nullptr, cap_entries, out->index, out->id, out->dist_sq);
        else if (out->offsets) query_enqueue_offsets(c, m, d_pref, d_wg);
        c->K.rev = rev;
        return SPHX_OK;
    }
    // host pointers.  scratch (64-bit words first): workgroup offsets [nblocks] | prefixes [m + 1] | count [1] | points [2m] | nearest [m] |
    // nearest_dist_sq [m]; the entries go to a second scratch sized once the total is known
    const size_t at_pref = 2 * (size_t)nblocks, at_cnt = at_pref + 2 * ((size_t)m + 1u), at_xy = at_cnt + 2, at_near = at_xy + 2 * (size_t)m;
    const size_t at_nd2 = at_near + (out->nearest ? (size_t)m : 0), words = at_nd2 + (out->nearest_dist_sq ? (size_t)m : 0);
    if ((rc = query_scratch(c, &c->query_buf, &c->query_cap, words))) return rc;
    uint32_t* const buf = c->query_buf;
    unsigned long long* const d_wg = (unsigned long long*)buf;
    unsigned long long* const d_pref = (unsigned long long*)(buf + at_pref);
    unsigned long long* const d_cnt = (unsigned long long*)(buf + at_cnt);
    float* const d_xy = (float*)(buf + at_xy);
    uint32_t* const d_near = out->nearest ? buf + at_near : nullptr;
    float* const d_nd2 = out->nearest_dist_sq ? (float*)(buf + at_nd2) : nullptr;
    hipError_t e = hipMemcpyAsync(d_xy, xy, 2 * (size_t)m * 4, hipMemcpyHostToDevice, st);
    unsigned long long total = 0;
    if (e == hipSuccess) {
        query_enqueue_count(c, a, d_xy, m, d_pref, d_wg, d_cnt, true, d_near, d_nd2);
        e = hipMemcpyAsync(&total, d_cnt, 8, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the one read of the total
    if (e != hipSuccess) {
        c->K.rev = rev;
        return c->fail(SPHX_ERR_HIP, fn, hipGetErrorString(e));
    }
    out->count[0] = total;
    const uint64_t got = std::min<uint64_t>(total, cap_entries);
    const bool walk2 = lists && got > 0u;
    uint32_t *d_index = nullptr, *d_id = nullptr;
    float* d_d2 = nullptr;
    if (walk2) {
        const size_t n_lists = (out->index ? 1u : 0u) + (out->id ? 1u : 0u) + (out->dist_sq ? 1u : 0u);
        if ((rc = query_scratch(c, &c->query_ent, &c->query_ent_cap, n_lists * (size_t)got))) {
            c->K.rev = rev;
            return rc;
        }
        uint32_t* p = c->query_ent;
        if (out->index) d_index = p, p += got;
        if (out->id) d_id = p, p += got;
        if (out->dist_sq) d_d2 = (float*)p;
        query_enqueue_emit(c, a, d_xy, m, d_pref, d_wg, d_cnt, true, got, d_index, d_id, d_d2);
    } else if (out->offsets) {
        query_enqueue_offsets(c, m, d_pref, d_wg);
    }
    c->K.rev = rev;
    if (out->offsets) SPHX_HIP(c, hipMemcpyAsync(out->offsets, d_pref, ((size_t)m + 1u) * 8, hipMemcpyDeviceToHost, st));
    if (d_near) SPHX_HIP(c, hipMemcpyAsync(out->nearest, d_near, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    if (d_nd2) SPHX_HIP(c, hipMemcpyAsync(out->nearest_dist_sq, d_nd2, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    if (d_index) SPHX_HIP(c, hipMemcpyAsync(out->index, d_index, (size_t)got * 4, hipMemcpyDeviceToHost, st));
    if (d_id) SPHX_HIP(c, hipMemcpyAsync(out->id, d_id, (size_t)got * 4, hipMemcpyDeviceToHost, st));
    if (d_d2) SPHX_HIP(c, hipMemcpyAsync(out->dist_sq, d_d2, (size_t)got * 4, hipMemcpyDeviceToHost, st));
    SPHX_HIP(c, hipStreamSynchronize(st));
    return SPHX_OK;
}

int sphx_select(sphx_ctx* c, const sphx_rect* rects, uint32_t n_rects, uint32_t flags, uint32_t cap, const sphx_select_out* out) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_select";
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out is NULL");
    if (!out->count) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out->count is NULL");
    if (n_rects > SPHX_REMOVE_MAX_RECTS) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "n_rects is larger than SPHX_REMOVE_MAX_RECTS");
    if (n_rects && !rects) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "rects is NULL with n_rects > 0");
    if (flags & ~(uint32_t)(SPHX_SELECT_OUTSIDE | SPHX_SELECT_DEVICE_POINTERS)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "unknown flags bits");
    sphx::EditRects R{};
    R.n = n_rects;
    R.outside = (flags & SPHX_SELECT_OUTSIDE) ? 0u : 1u;  // INVERTED: what sphx_remove's passes keep under R is what this call selects
    for (uint32_t k = 0; k < n_rects; ++k) {
        R.r[k] = rects[k];
        if (std::isnan(rects[k].x0) || std::isnan(rects[k].y0) || std::isnan(rects[k].x1) || std::isnan(rects[k].y1))
            return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "a rectangle bound is NaN (rects)");
    }
    if (c->tile_mode)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not available on a tile context (its arrays hold ghosts and miss the particles other tiles own)");
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, fn, "between step_begin and step_finish (finish the step first)");
    SPHX_HIP(c, hipSetDevice(c->device));
    flush_pending_advect(c);
    const bool device = (flags & SPHX_SELECT_DEVICE_POINTERS) != 0u;
    hipStream_t st = c->stream;
    const uint32_t n = c->N;
    if (n == 0) {
        if (device) SPHX_HIP(c, hipMemsetAsync(out->count, 0, 4, st));
        else out->count[0] = 0u;
        return SPHX_OK;
    }
    int rc;
    const uint32_t nb = (n + 255u) / 256u;
    if (nb + 1u > c->edit_cap) {
        SPHX_HIP(c, hipStreamSynchronize(st));
        if ((rc = dev_alloc(c, &c->edit_buf, (size_t)nb + 1u))) {
            c->edit_cap = 0;
            return rc;
        }
        c->edit_cap = nb + 1u;
    }
    const uint32_t rev = c->K.rev;  // (launch() toggles the sweep direction of the step's next kernels: put back below)
    uint32_t* const wg = c->edit_buf;
    launch(c, "select_flag", 8.0 * n + 4.0 * nb, [&] { hipLaunchKernelGGL(sphx::k_remove_flag, dim3(nb), dim3(256), 0, st, (const float2*)c->posA, n, R, wg); });
    launch(c, "select_scan", 8.0 * nb + 4.0, [&] { hipLaunchKernelGGL(sphx::k_remove_scan, dim3(1), dim3(256), 0, st, wg, nb); });
    const bool lists = out->index || out->id;
    if (device) {
        hipError_t e = hipMemcpyAsync(out->count, wg + nb, 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && lists && cap)
            launch(c, "select_emit", 8.0 * n + 4.0 * nb, [&] {
                hipLaunchKernelGGL(sphx::k_select_emit, dim3(nb), dim3(256), 0, st, (const float2*)c->posA, (const uint32_t*)c->pid, n, R, (const uint32_t*)wg, cap,
                                   out->index, out->id);
            });
        c->K.rev = rev;
        if (e != hipSuccess) return c->fail(SPHX_ERR_HIP, fn, hipGetErrorString(e));
        return SPHX_OK;
    }
    uint32_t total = 0;
    hipError_t e = hipMemcpyAsync(&total, wg + nb, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the one read of the total
    if (e != hipSuccess || total > n) {
        c->K.rev = rev;
        return c->fail(SPHX_ERR_HIP, fn, e != hipSuccess ? hipGetErrorString(e) : "the selection is larger than the particle count");
    }
    out->count[0] = total;
    const uint32_t got = std::min(total, cap);
    if (lists && got) {
        if ((rc = query_scratch(c, &c->query_ent, &c->query_ent_cap, 2 * (size_t)got))) {
            c->K.rev = rev;
            return rc;
        }
        uint32_t* const d_index = out->index ? c->query_ent : nullptr;
        uint32_t* const d_id = out->id ? c->query_ent + got : nullptr;
        launch(c, "select_emit", 8.0 * n + 4.0 * nb + 8.0 * got, [&] {
            hipLaunchKernelGGL(sphx::k_select_emit, dim3(nb), dim3(256), 0, st, (const float2*)c->posA, (const uint32_t*)c->pid, n, R, (const uint32_t*)wg, got, d_index,
                               d_id);
        });
        c->K.rev = rev;
        if (d_index) SPHX_HIP(c, hipMemcpyAsync(out->index, d_index, (size_t)got * 4, hipMemcpyDeviceToHost, st));
        if (d_id) SPHX_HIP(c, hipMemcpyAsync(out->id, d_id, (size_t)got * 4, hipMemcpyDeviceToHost, st));
        SPHX_HIP(c, hipStreamSynchronize(st));
    }
    c->K.rev = rev;
    return SPHX_OK;
}

// ---- one tile of a tiled run: the seam sphx_multi_query_radius / sphx_multi_select (sphx_tiles.cpp) are built on ------------------------
// Enqueue and fetch halves, like the sampling seam: the multi enqueues on every tile's stream first and then collects.

int sphx_tile_query_radius(sphx_ctx* c, const float* xy, uint32_t m, float radius, uint32_t flags, uint32_t want_nearest) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_query_radius";
    if (!c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not a tile context (sphx_query_radius serves a plain one)");
    if (m && !xy) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "xy is NULL with m > 0");
    if (flags & ~(uint32_t)SPHX_QUERY_BOUNDARY) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "unknown flags bits");
    if (m >= (1u << 31)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "m must be < 2^31");
    if (!std::isfinite(radius) || !(radius > 0.0f) || radius > c->P.smoothing_length)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "radius must be finite, > 0 and <= smoothing_length");
    c->tquery.stage = 0;
    c->tselect.stage = 0;
    c->tquery.m = m;
    if (m == 0) return SPHX_OK;
    int rc;
    if ((rc = tile_sample_state(c, fn))) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    const bool boundary = (flags & SPHX_QUERY_BOUNDARY) != 0u;
    sphx::QueryArgs a{};
    a.pos = (const float2*)c->posA;
    a.off = boundary ? c->soff() : 0u;
    a.ids = boundary ? (const uint32_t*)c->bid : (const uint32_t*)c->pid;
    const Grid& g = boundary ? c->gstat : c->gdyn;
    a.g = g.nview();
    a.r2 = radius * radius;
    a.empty = ((boundary ? c->B : c->N) == 0u || !g.dirn || !g.fine) ? 1u : 0u;  // (a tile without fluid answers with empty lists)
    // scratch (64-bit words first): workgroup offsets [nblocks] | prefixes [m + 1] | count [1] | points [2m] | owned points per selection
    // workgroup and their total [nblocks + 1, rounded up to even] | list [m] | nearest slot, id, dist_sq [m each]
    const uint32_t nblocks = (uint32_t)(((uint64_t)m + 255u) / 256u);
    sphx_ctx::TileQuery& q = c->tquery;
    q.at_pref = 2 * (size_t)nblocks;
    q.at_cnt = q.at_pref + 2 * ((size_t)m + 1u);
    q.at_xy = q.at_cnt + 2;
    q.at_own = q.at_xy + 2 * (size_t)m;
    q.at_list = q.at_own + (((size_t)nblocks + 2u) & ~(size_t)1u);
    q.at_near = q.at_list + (size_t)m;
    if ((rc = query_scratch(c, &c->query_buf, &c->query_cap, q.at_near + (want_nearest ? 3 * (size_t)m : 0)))) return rc;
    uint32_t* const buf = c->query_buf;
    hipStream_t st = c->stream;
    SPHX_HIP(c, hipMemcpyAsync(buf + q.at_xy, xy, 2 * (size_t)m * 4, hipMemcpyHostToDevice, st));
    const float2* const d_xy = (const float2*)(buf + q.at_xy);
    uint32_t* const own = buf + q.at_own;
    const uint32_t rev = c->K.rev;  // (launch() toggles the sweep direction of the step's next kernels: put back below)
    launch(c, "tile_query_own_flag", 8.0 * m + 4.0 * nblocks, [&] { hipLaunchKernelGGL(sphx::k_query_own_flag, dim3(nblocks), dim3(256), 0, st, c->K, d_xy, m, own); });
    launch(c, "tile_query_own_scan", 8.0 * nblocks + 4.0, [&] { hipLaunchKernelGGL(sphx::k_remove_scan, dim3(1), dim3(256), 0, st, own, nblocks); });
    launch(c, "tile_query_own_list", 12.0 * m + 4.0 * nblocks, [&] {
        hipLaunchKernelGGL(sphx::k_query_own_list, dim3(nblocks), dim3(256), 0, st, c->K, d_xy, m, (const uint32_t*)own, buf + q.at_list);
    });
    sphx::QueryList<true> L{buf + q.at_list, own + nblocks, want_nearest ? buf + q.at_near + m : nullptr, boundary ? 0xFFFFFFFFu : 0x7FFFFFFFu};
    query_enqueue_count(c, a, (const float*)d_xy, m, (unsigned long long*)(buf + q.at_pref), (unsigned long long*)buf, (unsigned long long*)(buf + q.at_cnt), true,
                        want_nearest ? buf + q.at_near : nullptr, want_nearest ? (float*)(buf + q.at_near + 2 * (size_t)m) : nullptr, &L);
    c->K.rev = rev;
    q.boundary = boundary ? 1u : 0u;
    q.nearest = want_nearest ? 1u : 0u;
    q.r2 = a.r2;
    q.nbp = nblocks;
    q.stage = 1;
    return SPHX_OK;
}

int sphx_tile_query_fetch(sphx_ctx* c, uint64_t cap_entries, sphx_tile_query_part* part) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_query_fetch";
    if (!part) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "part is NULL");
    if (!c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not a tile context");
    sphx_ctx::TileQuery& q = c->tquery;
    if (q.stage == 0) {  // (an empty query, or none: nothing was queued)
        part->n_points = 0;
        part->total = part->kept = 0;
        return SPHX_OK;
    }
    SPHX_HIP(c, hipSetDevice(c->device));
    uint32_t* const buf = c->query_buf;
    hipStream_t st = c->stream;
    const uint32_t m = q.m;
    int rc;
    if (q.stage == 1) {
        // the two totals with one synchronisation; then the entries and the final offsets go onto the stream
        uint32_t n_own = 0;
        unsigned long long total = 0;
        hipError_t e = hipMemcpyAsync(&n_own, buf + q.at_own + q.nbp, 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&total, buf + q.at_cnt, 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess || n_own > m) {
            q.stage = 0;
            return c->fail(SPHX_ERR_HIP, fn, e != hipSuccess ? hipGetErrorString(e) : "the list of owned points is longer than the point set");
        }
        q.n_own = n_own;
        q.total = total;
        q.kept = std::min<uint64_t>(total, cap_entries);
        unsigned long long* const d_wg = (unsigned long long*)buf;
        unsigned long long* const d_pref = (unsigned long long*)(buf + q.at_pref);
        const uint32_t rev = c->K.rev;
        if (n_own && q.kept) {
            // the entry scratch holds min(tile total, cap_entries): an entry's position in the merged list is never below its position here
            if ((rc = query_scratch(c, &c->query_ent, &c->query_ent_cap, 3 * (size_t)q.kept))) {
                q.stage = 0;
                return rc;
            }
            sphx::QueryArgs a{};
            const bool boundary = q.boundary != 0u;
            a.pos = (const float2*)c->posA;
            a.off = boundary ? c->soff() : 0u;
            a.ids = boundary ? (const uint32_t*)c->bid : (const uint32_t*)c->pid;
            a.g = (boundary ? c->gstat : c->gdyn).nview();
            a.r2 = q.r2;
            a.empty = 0u;  // (kept > 0: the set is not empty)
            sphx::QueryList<true> L{buf + q.at_list, buf + q.at_own + q.nbp, nullptr, boundary ? 0xFFFFFFFFu : 0x7FFFFFFFu};
            query_enqueue_emit(c, a, (const float*)(buf + q.at_xy), m, d_pref, d_wg, (const unsigned long long*)(buf + q.at_cnt), true, q.kept, c->query_ent,
                               c->query_ent + q.kept, (float*)(c->query_ent + 2 * q.kept), &L);
        } else if (n_own) {
            query_enqueue_offsets(c, n_own, d_pref, d_wg);
        }
        c->K.rev = rev;
        q.stage = 2;
    }
    part->n_points = q.n_own;
    part->total = q.total;
    part->kept = q.kept;
    if (!part->point && !part->offset) return SPHX_OK;  // the sizes alone: the caller allocates and comes back
    const size_t n = q.n_own;
    q.stage = 0;
    if (n) {
        if (part->point) SPHX_HIP(c, hipMemcpyAsync(part->point, buf + q.at_list, n * 4, hipMemcpyDeviceToHost, st));
        if (part->offset) SPHX_HIP(c, hipMemcpyAsync(part->offset, buf + q.at_pref, n * 8, hipMemcpyDeviceToHost, st));
        if (q.nearest) {
            if (part->nearest_slot) SPHX_HIP(c, hipMemcpyAsync(part->nearest_slot, buf + q.at_near, n * 4, hipMemcpyDeviceToHost, st));
            if (part->nearest_id) SPHX_HIP(c, hipMemcpyAsync(part->nearest_id, buf + q.at_near + m, n * 4, hipMemcpyDeviceToHost, st));
            if (part->nearest_dist_sq) SPHX_HIP(c, hipMemcpyAsync(part->nearest_dist_sq, buf + q.at_near + 2 * (size_t)m, n * 4, hipMemcpyDeviceToHost, st));
        }
        if (q.kept) {
            if (part->slot) SPHX_HIP(c, hipMemcpyAsync(part->slot, c->query_ent, (size_t)q.kept * 4, hipMemcpyDeviceToHost, st));
            if (part->id) SPHX_HIP(c, hipMemcpyAsync(part->id, c->query_ent + q.kept, (size_t)q.kept * 4, hipMemcpyDeviceToHost, st));
            if (part->dist_sq) SPHX_HIP(c, hipMemcpyAsync(part->dist_sq, c->query_ent + 2 * q.kept, (size_t)q.kept * 4, hipMemcpyDeviceToHost, st));
        }
        SPHX_HIP(c, hipStreamSynchronize(st));
    }
    return SPHX_OK;
}

int sphx_tile_select(sphx_ctx* c, const sphx_rect* rects, uint32_t n_rects, uint32_t flags) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_select";
    if (!c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not a tile context (sphx_select serves a plain one)");
    if (n_rects > SPHX_REMOVE_MAX_RECTS) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "n_rects is larger than SPHX_REMOVE_MAX_RECTS");
    if (n_rects && !rects) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "rects is NULL with n_rects > 0");
    if (flags & ~(uint32_t)SPHX_SELECT_OUTSIDE) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "unknown flags bits");
    for (uint32_t k = 0; k < n_rects; ++k)
        if (std::isnan(rects[k].x0) || std::isnan(rects[k].y0) || std::isnan(rects[k].x1) || std::isnan(rects[k].y1))
            return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "a rectangle bound is NaN (rects)");
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, fn, "between step_begin and step_finish (finish the step first)");
    sphx_ctx::TileSelect& s = c->tselect;
    c->tquery.stage = 0;
    s.stage = 0;
    s.n_rects = n_rects;
    s.outside = (flags & SPHX_SELECT_OUTSIDE) ? 0u : 1u;  // INVERTED, as in sphx_select
    for (uint32_t k = 0; k < n_rects; ++k) s.r[k] = rects[k];
    SPHX_HIP(c, hipSetDevice(c->device));
    flush_pending_advect(c);
    const uint32_t n = c->N;
    s.n = n;
    s.total = 0;
    if (n == 0) {
        s.stage = 2;
        return SPHX_OK;
    }
    int rc;
    const uint32_t nb = (n + 255u) / 256u;
    if (nb + 1u > c->edit_cap) {
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
        if ((rc = dev_alloc(c, &c->edit_buf, (size_t)nb + 1u))) {
            c->edit_cap = 0;
            return rc;
        }
        c->edit_cap = nb + 1u;
    }
    sphx::EditRects R{};
    R.n = n_rects;
    R.outside = s.outside;
    for (uint32_t k = 0; k < n_rects; ++k) R.r[k] = rects[k];
    hipStream_t st = c->stream;
    uint32_t* const wg = c->edit_buf;
    const uint32_t rev = c->K.rev;
    launch(c, "tile_select_flag", 12.0 * n + 4.0 * nb, [&] {
        hipLaunchKernelGGL(sphx::k_tile_select_flag, dim3(nb), dim3(256), 0, st, (const float2*)c->posA, (const uint32_t*)c->pid, n, R, wg);
    });
    launch(c, "tile_select_scan", 8.0 * nb + 4.0, [&] { hipLaunchKernelGGL(sphx::k_remove_scan, dim3(1), dim3(256), 0, st, wg, nb); });
    c->K.rev = rev;
    s.nb = nb;
    s.stage = 1;
    return SPHX_OK;
}

int sphx_tile_select_fetch(sphx_ctx* c, uint32_t cap, uint32_t* slot, uint32_t* id, uint32_t* out_total) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_select_fetch";
    if (!out_total) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out_total is NULL");
    *out_total = 0;
    if (!c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not a tile context");
    sphx_ctx::TileSelect& s = c->tselect;
    if (s.stage == 0) return c->fail(SPHX_ERR_NOT_READY, fn, "no sphx_tile_select is queued");
    SPHX_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (s.stage == 1) {
        uint32_t total = 0;
        hipError_t e = hipMemcpyAsync(&total, c->edit_buf + s.nb, 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);  // the one read of the total
        if (e != hipSuccess || total > s.n) {
            s.stage = 0;
            return c->fail(SPHX_ERR_HIP, fn, e != hipSuccess ? hipGetErrorString(e) : "the selection is larger than the particle count");
        }
        s.total = total;
        s.stage = 2;
    }
    *out_total = s.total;
    const uint32_t got = std::min(s.total, cap);
    if (!got || (!slot && !id)) return SPHX_OK;  // the total alone: the caller sizes its arrays and comes back
    if (s.n != c->N) {
        s.stage = 0;
        return c->fail(SPHX_ERR_NOT_READY, fn, "the particle set changed since sphx_tile_select");
    }
    int rc;
    if ((rc = query_scratch(c, &c->query_ent, &c->query_ent_cap, 2 * (size_t)got))) return rc;
    sphx::EditRects R{};
    R.n = s.n_rects;
    R.outside = s.outside;
    for (uint32_t k = 0; k < s.n_rects; ++k) R.r[k] = s.r[k];
    uint32_t* const d_slot = c->query_ent;
    uint32_t* const d_id = c->query_ent + got;
    const uint32_t rev = c->K.rev;
    launch(c, "tile_select_emit", 12.0 * s.n + 4.0 * s.nb + 8.0 * got, [&] {
        hipLaunchKernelGGL(sphx::k_tile_select_emit, dim3(s.nb), dim3(256), 0, st, (const float2*)c->posA, (const uint32_t*)c->pid, s.n, R, (const uint32_t*)c->edit_buf, got,
                           d_slot, d_id);
    });
    c->K.rev = rev;
    if (slot) SPHX_HIP(c, hipMemcpyAsync(slot, d_slot, (size_t)got * 4, hipMemcpyDeviceToHost, st));
    if (id) SPHX_HIP(c, hipMemcpyAsync(id, d_id, (size_t)got * 4, hipMemcpyDeviceToHost, st));
    SPHX_HIP(c, hipStreamSynchronize(st));
    return SPHX_OK;
}

}  // extern "C"
