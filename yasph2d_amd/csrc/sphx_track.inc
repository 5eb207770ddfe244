// sphx_track.inc — following particles by id (sphx_track_*, sphx_download_by_id, include/sphx.h): the slot of an id, found on the device,
// instead of a full download and an argsort on the host.  Included at the end of sphx_kernels.hip (one translation unit: the launch
// layer of sphx_launch.inc is visible).  The host half of a tracked set (sorting, the map, the filter, the argument checks) is
// sphx_track_set.hpp.  Everything here only READS the particle state: nothing a step reads is written (DESIGN.md §4g).
#include "sphx_track_set.hpp"
#include "sphx_track_merge.hpp"

namespace sphx {

typedef uint32_t track_u32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t TRACK_CHUNK = 1024;     // particles per workgroup and trip: one 16-byte load of pid[] per lane
constexpr uint32_t TRACK_MAX_GRID = 2048;  // look-up workgroups per launch: each stages the filter once and strides over the chunks
constexpr uint32_t TRACK_WINDOW = 1u << 22;  // sphx_download_by_id: ids per pass (16 MiB of index, 112 MiB of outputs on the host-pointer path)
constexpr uint32_t TRACK_NT_FROM = 4000000u;  // pid[] is read once and by nobody else soon: nontemporal loads from here (as the lists, NbView::stream)

struct TrackTable {
    const uint32_t* table;   // [unique] ascending
    const uint32_t* filter;  // 2^log2_bits bits
    uint32_t* found;         // [unique] slot + 1 of the highest slot that carries the id, 0 = none (cleared on the stream before the pass)
    uint32_t unique, log2_bits;
};

// One particle: filter bit (LDS), then the binary search of the L2-resident table, then the integer maximum of slot + 1.  The filter only
// saves probes: a lane that passes it by accident finds nothing in the table.
__device__ __forceinline__ void track_probe(const TrackTable& T, const uint32_t* filter, uint32_t id, uint32_t slot) {
    const uint32_t b = track_hash(id, T.log2_bits);
    if (!((filter[b >> 5] >> (b & 31u)) & 1u)) return;
    uint32_t lo = 0, hi = T.unique;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (T.table[mid] < id) lo = mid + 1u;
        else hi = mid;
    }
    if (lo < T.unique && T.table[lo] == id) atomicMax(&T.found[lo], slot + 1u);
}

// The look-up pass: one streaming sweep over pid[], 4 bytes per particle.  Workgroups are taken in blockIdx.x order with a grid stride
// (not xcd_bid(): nothing is re-read by a neighbouring kernel, and the result does not depend on the order — an integer maximum).
// Dynamic LDS: the filter, 2^log2_bits / 8 bytes (128 B ... 32 KiB).
//   OWNED (one tile of a tiled run, sphx_tile_track_*): a particle only answers if bit 31 of its pid word is set (the tile owns it), for
// the other 31 bits; a ghost is never probed.  Without OWNED the kernel is the single context's, instruction for instruction.
template <bool OWNED>
__device__ __forceinline__ void track_probe_word(const TrackTable& T, const uint32_t* filter, uint32_t w, uint32_t slot) {
    if (OWNED) {
        if (w >> 31) track_probe(T, filter, w & 0x7FFFFFFFu, slot);
    } else {
        track_probe(T, filter, w, slot);
    }
}
template <bool NT, bool OWNED = false>
__global__ __launch_bounds__(256) void k_track_lookup(const uint32_t* __restrict__ pid, uint32_t n, TrackTable T) {
    extern __shared__ uint32_t track_filter_lds[];
    const uint32_t words = 1u << (T.log2_bits - 5u);
    for (uint32_t w = threadIdx.x; w < words; w += 256u) track_filter_lds[w] = T.filter[w];
    __syncthreads();
    const uint32_t chunks = (n + TRACK_CHUNK - 1u) / TRACK_CHUNK;  // (n < 2^28: no overflow below)
    for (uint32_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const uint32_t i0 = ch * TRACK_CHUNK + threadIdx.x * 4u;
        if (i0 + 4u <= n) {
            const track_u32x4* p = (const track_u32x4*)(pid + i0);  // (pid is a device allocation of its own and i0 a multiple of 4: 16-byte aligned)
            const track_u32x4 v = NT ? __builtin_nontemporal_load(p) : *p;
            track_probe_word<OWNED>(T, track_filter_lds, v.x, i0);
            track_probe_word<OWNED>(T, track_filter_lds, v.y, i0 + 1u);
            track_probe_word<OWNED>(T, track_filter_lds, v.z, i0 + 2u);
            track_probe_word<OWNED>(T, track_filter_lds, v.w, i0 + 3u);
        } else {
            for (uint32_t k = 0; k < 4u; ++k)
                if (i0 + k < n) track_probe_word<OWNED>(T, track_filter_lds, pid[i0 + k], i0 + k);
        }
    }
}

// sphx_download_by_id, pass 1: every particle whose id lies in [first_id, first_id + count) leaves slot + 1 in index[id - first_id]
// (first_id + count <= 2^32, so an id below the window wraps to a difference >= count)
template <bool NT>
__global__ __launch_bounds__(256) void k_track_window(const uint32_t* __restrict__ pid, uint32_t n, uint32_t first_id, uint32_t count,
                                                      uint32_t* __restrict__ index) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t d = (NT ? __builtin_nontemporal_load(pid + i) : pid[i]) - first_id;
    if (d < count) atomicMax(&index[d], i + 1u);
}

// The by-id download of one tile (sphx_tile_track_window_enqueue): every OWNED particle whose id lies in the window appends one packed
// 32-byte record {id - first_id, slot, x, y, vx, vy, density, 0} behind the tile's counter head[0].  pid[] is streamed as in
// k_track_lookup, four particles per lane and trip.  A wavefront reserves its records with ONE atomic per trip: four ballots (one per
// particle of a lane), their population counts, one atomicAdd of the sum by lane 0, then per lane the prefix of its ballot.  The loop
// bounds are workgroup-uniform, so all 64 lanes are active at the ballots.  The order of the records is whatever the atomics give; the
// host scatter does not depend on it.  A position at or beyond `cap` is never written — the counter still counts it, and the host
// reports the overflow.
template <bool NT>
__global__ __launch_bounds__(256) void k_track_window_owned(const uint32_t* __restrict__ pid, uint32_t n, uint32_t first_id, uint32_t count,
                                                            const uint2* __restrict__ pos, const uint2* __restrict__ vel,
                                                            const uint32_t* __restrict__ density, uint32_t* __restrict__ head,
                                                            uint4* __restrict__ rec, uint32_t cap) {
    const uint32_t chunks = (n + TRACK_CHUNK - 1u) / TRACK_CHUNK;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const uint32_t i0 = ch * TRACK_CHUNK + threadIdx.x * 4u;
        uint32_t w[4] = {0u, 0u, 0u, 0u};  // (a word without bit 31 never answers: what a lane beyond n holds)
        if (i0 + 4u <= n) {
            const track_u32x4* p = (const track_u32x4*)(pid + i0);
            const track_u32x4 v = NT ? __builtin_nontemporal_load(p) : *p;
            w[0] = v.x;
            w[1] = v.y;
            w[2] = v.z;
            w[3] = v.w;
        } else {
            for (uint32_t k = 0; k < 4u; ++k)
                if (i0 + k < n) w[k] = pid[i0 + k];
        }
        bool hit[4];
        unsigned long long b[4];
        uint32_t total = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            // (first_id + count <= 2^32 and the masked id < 2^31: an id below the window wraps to a difference >= count)
            hit[k] = (w[k] >> 31) && ((w[k] & 0x7FFFFFFFu) - first_id) < count;
            b[k] = __ballot(hit[k]);
            total += (uint32_t)__popcll(b[k]);
        }
        if (!total) continue;  // (wave-uniform)
        uint32_t base = 0;
        if (lane == 0u) base = atomicAdd(head, total);
        base = __shfl(base, 0);
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t at = base + (uint32_t)__popcll(b[k] & below);
            base += (uint32_t)__popcll(b[k]);
            if (!hit[k] || at >= cap) continue;
            const uint32_t j = i0 + k;
            const uint2 p = pos[j], v = vel[j];
            rec[2 * (size_t)at] = make_uint4((w[k] & 0x7FFFFFFFu) - first_id, j, p.x, p.y);
            rec[2 * (size_t)at + 1] = make_uint4(v.x, v.y, density[j], 0u);
        }
    }
}

// The second, small launch of both calls: output k takes the records at slot found[map[k]] - 1 (map == nullptr: found[k]), or the absent
// words.  All in 32-bit integer words: the outputs are the bits sphx_download returns, whatever they encode.  The outputs may be the
// caller's device arrays, so only 4-byte alignment is assumed for them; a frame is the library's own buffer (16-byte records).
struct TrackEmit {
    const uint32_t* found;
    const uint32_t* map;
    uint32_t m;
    const uint2* pos;        // posA
    const uint2* vel;
    const uint32_t* density;
    uint32_t* o_slot;        // [m] or null
    uint32_t* o_pos;         // [2m] or null
    uint32_t* o_vel;         // [2m] or null
    uint32_t* o_density;     // [m] or null
    uint4* o_frame;          // [m] {x, y, vx, vy} or null
    uint32_t* o_present;     // one counter the found ones are added to, or null
};
__global__ __launch_bounds__(256) void k_track_emit(TrackEmit e) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const bool live = k < e.m;
    const uint32_t f = live ? e.found[e.map ? e.map[k] : k] : 0u;
    const bool present = f != 0u;
    if (e.o_present) {
        const unsigned long long b = __ballot(present);
        if ((threadIdx.x & 63u) == 0u && b) atomicAdd(e.o_present, (uint32_t)__popcll(b));
    }
    if (!live) return;
    const uint32_t j = f - 1u;  // (< n: written by a lane that held particle j)
    const uint32_t A = TRACK_ABSENT_WORD;
    uint2 p = make_uint2(A, A), v = make_uint2(A, A);
    if (present && (e.o_pos || e.o_frame)) p = e.pos[j];
    if (present && (e.o_vel || e.o_frame)) v = e.vel[j];
    if (e.o_slot) e.o_slot[k] = present ? j : TRACK_ABSENT;
    if (e.o_pos) {
        e.o_pos[2 * (size_t)k] = p.x;
        e.o_pos[2 * (size_t)k + 1] = p.y;
    }
    if (e.o_vel) {
        e.o_vel[2 * (size_t)k] = v.x;
        e.o_vel[2 * (size_t)k + 1] = v.y;
    }
    if (e.o_density) e.o_density[k] = present ? e.density[j] : A;
    if (e.o_frame) e.o_frame[k] = make_uint4(p.x, p.y, v.x, v.y);
}

}  // namespace sphx

// ---- launch layer and C ABI ----------------------------------------------------------------------------------------------------------
namespace {

// the arguments every call checks after its own: a tile context is refused as an argument, an open step as a state
int track_check_ctx(sphx_ctx* c, const char* fn) {
    const std::string f = fn;
    if (c->tile_mode)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": not available on a tile context (its arrays hold ghosts and its ids need not be unique)").c_str());
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, (f + ": between step_begin and step_finish (finish the step first)").c_str());
    return SPHX_OK;
}
int track_check_out(sphx_ctx* c, const char* fn, uint32_t flags, const sphx_track_out* out) {
    const std::string f = fn;
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": out is NULL").c_str());
    if (!out->slot && !out->pos && !out->vel && !out->density)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": out requests no output (every pointer is NULL)").c_str());
    if (flags & ~(uint32_t)SPHX_TRACK_DEVICE_POINTERS) return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": unknown flags bits").c_str());
    return SPHX_OK;
}

void track_drop_recording(sphx_ctx* c) {
    sphx_ctx::Track& t = c->track;
    dev_free(&t.rec);
    t.recording = t.max_frames = t.every = t.frames = t.dropped = t.steps = 0;
}

int track_scratch(sphx_ctx* c, size_t words) {
    sphx_ctx::Track& t = c->track;
    if (words <= t.scratch_cap) return SPHX_OK;
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    int rc;
    if ((rc = dev_alloc(c, &t.scratch, words))) {
        t.scratch_cap = 0;
        return rc;
    }
    t.scratch_cap = words;
    return SPHX_OK;
}

TrackEmit track_emit_args(const sphx_ctx* c, const uint32_t* found, const uint32_t* map, uint32_t m) {
    TrackEmit e{};
    e.found = found;
    e.map = map;
    e.m = m;
    e.pos = (const uint2*)c->posA;
    e.vel = (const uint2*)c->vel;
    e.density = (const uint32_t*)c->density;
    return e;
}
void track_set_out(TrackEmit& e, const sphx_track_out& o, size_t at) {
    e.o_slot = o.slot ? o.slot + at : nullptr;
    e.o_pos = o.pos ? (uint32_t*)o.pos + 2 * at : nullptr;
    e.o_vel = o.vel ? (uint32_t*)o.vel + 2 * at : nullptr;
    e.o_density = o.density ? (uint32_t*)o.density + at : nullptr;
}
void track_enqueue_emit(sphx_ctx* c, const TrackEmit& e) {
    hipStream_t st = c->stream;
    launch(c, "track_emit", 8.0 * e.m + 28.0 * e.m, [&] { hipLaunchKernelGGL(k_track_emit, dim3((e.m + 255u) / 256u), dim3(256), 0, st, e); });
}

// found[] of the tracked set for the arrays as they are now: a memset and the sweep over pid[] (none for an empty context)
int track_enqueue_lookup(sphx_ctx* c) {
    sphx_ctx::Track& t = c->track;
    hipStream_t st = c->stream;
    SPHX_HIP(c, hipMemsetAsync(t.found, 0, (size_t)t.unique * 4, st));
    const uint32_t n = c->N;
    if (!n) return SPHX_OK;
    const TrackTable T{t.table, t.filter, t.found, t.unique, t.log2_bits};
    const uint32_t grid = std::min((n + TRACK_CHUNK - 1u) / TRACK_CHUNK, TRACK_MAX_GRID);
    const uint32_t lds = (1u << t.log2_bits) / 8u;
    launch(c, "track_lookup", 4.0 * n, [&] {
        if (n >= TRACK_NT_FROM)
            hipLaunchKernelGGL(k_track_lookup<true>, dim3(grid), dim3(256), lds, st, (const uint32_t*)c->pid, n, T);
        else
            hipLaunchKernelGGL(k_track_lookup<false>, dim3(grid), dim3(256), lds, st, (const uint32_t*)c->pid, n, T);
    });
    return SPHX_OK;
}

// One frame behind the kernels of the step that has just finished (sphx_step_finish / sphx_wcsph_step_finish call this through
// track_after_step when a recording is on).  Nothing comes back to the host; an enqueue error only loses the frame.
void track_take_frame(sphx_ctx* c) {
    sphx_ctx::Track& t = c->track;
    if (c->tile_mode || !t.m) return;
    if (++t.steps % t.every) return;
    if (t.frames >= t.max_frames) {
        t.dropped += 1u;
        return;
    }
    const uint32_t rev = c->K.rev;  // (the recorder must not change the sweep direction of the next step's kernels: launch() toggles it)
    if (track_enqueue_lookup(c) == SPHX_OK) {
        TrackEmit e = track_emit_args(c, t.found, t.map, t.m);
        e.o_frame = (uint4*)t.rec + (size_t)t.frames * t.m;
        track_enqueue_emit(c, e);
        t.frames += 1u;
    } else {
        t.dropped += 1u;
    }
    c->K.rev = rev;
}

}  // namespace

extern "C" {

int sphx_track_set(sphx_ctx* c, const uint32_t* ids, uint32_t m) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (const char* bad = track_check_ids(ids, m)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_track_set", bad);
    int rc;
    if ((rc = track_check_ctx(c, "sphx_track_set"))) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));  // (a queued frame or fetch may still read the old tables)
    sphx_ctx::Track& t = c->track;
    track_drop_recording(c);
    t.m = t.unique = 0;
    if (m == 0) {
        dev_free(&t.set_buf);
        t.table = t.map = t.filter = t.found = nullptr;
        return SPHX_OK;
    }
    const TrackSet s = track_build(ids, m);
    const size_t u = s.unique(), fw = s.filter.size();
    if ((rc = dev_alloc(c, &t.set_buf, u + m + fw + u))) return rc;
    t.table = t.set_buf;
    t.map = t.table + u;
    t.filter = t.map + m;
    t.found = t.filter + fw;
    SPHX_HIP(c, hipMemcpyAsync(t.table, s.table.data(), u * 4, hipMemcpyHostToDevice, c->stream));
    SPHX_HIP(c, hipMemcpyAsync(t.map, s.map.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
    SPHX_HIP(c, hipMemcpyAsync(t.filter, s.filter.data(), fw * 4, hipMemcpyHostToDevice, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));  // (the host tables go away with this call)
    t.m = m;
    t.unique = (uint32_t)u;
    t.log2_bits = s.log2_bits;
    return SPHX_OK;
}

int sphx_track_fetch(sphx_ctx* c, uint32_t flags, const sphx_track_out* out) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = track_check_out(c, "sphx_track_fetch", flags, out))) return rc;
    if ((rc = track_check_ctx(c, "sphx_track_fetch"))) return rc;
    sphx_ctx::Track& t = c->track;
    const uint32_t m = t.m;
    if (m == 0) return SPHX_OK;
    SPHX_HIP(c, hipSetDevice(c->device));
    const bool dev = flags & SPHX_TRACK_DEVICE_POINTERS;
    const size_t n_s = out->slot ? m : 0, n_p = out->pos ? 2 * (size_t)m : 0, n_v = out->vel ? 2 * (size_t)m : 0, n_d = out->density ? m : 0;
    sphx_track_out o = *out;
    if (!dev) {
        if ((rc = track_scratch(c, n_s + n_p + n_v + n_d))) return rc;
        uint32_t* p = t.scratch;
        o.slot = out->slot ? p : nullptr;
        p += n_s;
        o.pos = out->pos ? (float*)p : nullptr;
        p += n_p;
        o.vel = out->vel ? (float*)p : nullptr;
        p += n_v;
        o.density = out->density ? (float*)p : nullptr;
    }
    const uint32_t rev = c->K.rev;  // (a fetch must not change the sweep direction of the step's next kernels: launch() toggles it)
    rc = track_enqueue_lookup(c);
    if (rc == SPHX_OK) {
        TrackEmit e = track_emit_args(c, t.found, t.map, m);
        track_set_out(e, o, 0);
        track_enqueue_emit(c, e);
    }
    c->K.rev = rev;
    if (rc || dev) return rc;
    hipStream_t st = c->stream;
    if (n_s) SPHX_HIP(c, hipMemcpyAsync(out->slot, o.slot, n_s * 4, hipMemcpyDeviceToHost, st));
    if (n_p) SPHX_HIP(c, hipMemcpyAsync(out->pos, o.pos, n_p * 4, hipMemcpyDeviceToHost, st));
    if (n_v) SPHX_HIP(c, hipMemcpyAsync(out->vel, o.vel, n_v * 4, hipMemcpyDeviceToHost, st));
    if (n_d) SPHX_HIP(c, hipMemcpyAsync(out->density, o.density, n_d * 4, hipMemcpyDeviceToHost, st));
    SPHX_HIP(c, hipStreamSynchronize(st));
    return SPHX_OK;
}

int sphx_track_record(sphx_ctx* c, uint32_t max_frames, uint32_t every) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = track_check_ctx(c, "sphx_track_record"))) return rc;
    sphx_ctx::Track& t = c->track;
    bool capacity = false;
    if (max_frames) {  // (max_frames == 0 stops and frees, whatever `every` says)
        if (const char* bad = track_check_record(t.m, max_frames, every, &capacity))
            return c->fail(capacity ? SPHX_ERR_CAPACITY : SPHX_ERR_INVALID_ARGUMENT, "sphx_track_record", bad);
        if (!t.m) return c->fail(SPHX_ERR_NOT_READY, "sphx_track_record: the tracked set is empty (call sphx_track_set first)");
    }
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));  // (a queued frame may still write the old buffer)
    track_drop_recording(c);
    if (!max_frames) return SPHX_OK;
    if ((rc = dev_alloc(c, &t.rec, (size_t)max_frames * t.m * 4))) return rc;
    t.max_frames = max_frames;
    t.every = every;
    t.recording = 1u;
    return SPHX_OK;
}

int sphx_track_get_status(const sphx_ctx* c, sphx_track_status* out) {
    if (!c || !out) return SPHX_ERR_INVALID_ARGUMENT;
    const sphx_ctx::Track& t = c->track;
    std::memset(out, 0, sizeof(*out));
    out->m = t.m;
    out->recording = t.recording;
    out->max_frames = t.max_frames;
    out->every = t.every;
    out->frames = t.frames;
    out->dropped = t.dropped;
    return SPHX_OK;
}

int sphx_track_read(sphx_ctx* c, uint32_t first_frame, uint32_t n_frames, uint32_t flags, float* out) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (flags & ~(uint32_t)SPHX_TRACK_DEVICE_POINTERS) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_track_read: unknown flags bits");
    int rc;
    if ((rc = track_check_ctx(c, "sphx_track_read"))) return rc;
    const sphx_ctx::Track& t = c->track;
    if ((uint64_t)first_frame + n_frames > t.frames)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_track_read: first_frame + n_frames is beyond the frames recorded (sphx_track_get_status)");
    if (n_frames == 0) return SPHX_OK;
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_track_read: out is NULL");
    SPHX_HIP(c, hipSetDevice(c->device));
    const size_t frame = (size_t)t.m * 16;
    const bool dev = flags & SPHX_TRACK_DEVICE_POINTERS;
    SPHX_HIP(c, hipMemcpyAsync(out, (const char*)t.rec + first_frame * frame, n_frames * frame, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                               c->stream));
    if (!dev) SPHX_HIP(c, hipStreamSynchronize(c->stream));
    return SPHX_OK;
}

int sphx_download_by_id(sphx_ctx* c, uint32_t first_id, uint32_t count, uint32_t flags, const sphx_track_out* out, uint32_t* out_present) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = track_check_out(c, "sphx_download_by_id", flags, out))) return rc;
    if (const char* bad = track_check_range(first_id, count)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_download_by_id", bad);
    if ((rc = track_check_ctx(c, "sphx_download_by_id"))) return rc;
    const bool dev = flags & SPHX_TRACK_DEVICE_POINTERS;
    if (count == 0) {
        if (out_present && !dev) *out_present = 0;
        if (out_present && dev) {
            SPHX_HIP(c, hipSetDevice(c->device));
            SPHX_HIP(c, hipMemsetAsync(out_present, 0, 4, c->stream));
        }
        return SPHX_OK;
    }
    SPHX_HIP(c, hipSetDevice(c->device));
    sphx_ctx::Track& t = c->track;
    // scratch: the present counter (4 words: the index stays 16-byte aligned), the window's index, and on the host-pointer path the outputs
    const uint32_t win = std::min(count, TRACK_WINDOW);
    const size_t n_s = out->slot ? win : 0, n_p = out->pos ? 2 * (size_t)win : 0, n_v = out->vel ? 2 * (size_t)win : 0, n_d = out->density ? win : 0;
    if ((rc = track_scratch(c, 4 + (size_t)win + (dev ? 0 : n_s + n_p + n_v + n_d)))) return rc;
    uint32_t* const present = t.scratch;
    uint32_t* const index = t.scratch + 4;
    sphx_track_out o{};
    if (!dev) {
        uint32_t* p = index + win;
        o.slot = out->slot ? p : nullptr;
        p += n_s;
        o.pos = out->pos ? (float*)p : nullptr;
        p += n_p;
        o.vel = out->vel ? (float*)p : nullptr;
        p += n_v;
        o.density = out->density ? (float*)p : nullptr;
    }
    hipStream_t st = c->stream;
    const uint32_t n = c->N;
    const uint32_t rev = c->K.rev;
    auto done = [&](int code) {
        c->K.rev = rev;
        return code;
    };
    SPHX_HIP(c, hipMemsetAsync(present, 0, 4, st));
    for (uint64_t w0 = 0; w0 < count; w0 += TRACK_WINDOW) {
        const uint32_t wc = (uint32_t)std::min<uint64_t>(count - w0, TRACK_WINDOW);
        const uint32_t wfirst = first_id + (uint32_t)w0;
        if (hipMemsetAsync(index, 0, (size_t)wc * 4, st) != hipSuccess) return done(c->fail(SPHX_ERR_HIP, "sphx_download_by_id: hipMemsetAsync"));
        if (n)
            launch(c, "track_window", 4.0 * n, [&] {
                if (n >= TRACK_NT_FROM)
                    hipLaunchKernelGGL(k_track_window<true>, dim3((n + 255u) / 256u), dim3(256), 0, st, (const uint32_t*)c->pid, n, wfirst, wc, index);
                else
                    hipLaunchKernelGGL(k_track_window<false>, dim3((n + 255u) / 256u), dim3(256), 0, st, (const uint32_t*)c->pid, n, wfirst, wc, index);
            });
        TrackEmit e = track_emit_args(c, index, nullptr, wc);
        track_set_out(e, dev ? *out : o, dev ? (size_t)w0 : 0);
        e.o_present = present;
        track_enqueue_emit(c, e);
        if (!dev) {
            hipError_t he = hipSuccess;
            if (out->slot && he == hipSuccess) he = hipMemcpyAsync(out->slot + w0, o.slot, (size_t)wc * 4, hipMemcpyDeviceToHost, st);
            if (out->pos && he == hipSuccess) he = hipMemcpyAsync(out->pos + 2 * w0, o.pos, (size_t)wc * 8, hipMemcpyDeviceToHost, st);
            if (out->vel && he == hipSuccess) he = hipMemcpyAsync(out->vel + 2 * w0, o.vel, (size_t)wc * 8, hipMemcpyDeviceToHost, st);
            if (out->density && he == hipSuccess) he = hipMemcpyAsync(out->density + w0, o.density, (size_t)wc * 4, hipMemcpyDeviceToHost, st);
            if (he != hipSuccess) return done(c->fail(SPHX_ERR_HIP, "sphx_download_by_id: copy to the host", hipGetErrorString(he)));
        }
    }
    c->K.rev = rev;
    if (dev) {
        if (out_present) SPHX_HIP(c, hipMemcpyAsync(out_present, present, 4, hipMemcpyDeviceToDevice, st));
        return SPHX_OK;
    }
    if (out_present) SPHX_HIP(c, hipMemcpyAsync(out_present, present, 4, hipMemcpyDeviceToHost, st));
    SPHX_HIP(c, hipStreamSynchronize(st));
    return SPHX_OK;
}

}  // extern "C"

// ---- one tile of a tiled run (sphx_multi_track_*, sphx_multi_download_by_id, sphx_tiles.cpp, are built on these) ------------------------
// A tile keeps its tables in the context's Track too: table | filter | found of ONE track_build shared by all tiles, m = unique (the
// map to the caller's order stays on the host, with the multi).  Only owned particles answer (k_track_lookup<NT, true>).
namespace {

static_assert(TRACK_WINDOW == sphx_track_host::WINDOW, "the window of the by-id download, device and host");

int track_check_tile(sphx_ctx* c, const char* fn) {
    const std::string f = fn;
    if (!c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": not a tile context (sphx_track_* and sphx_download_by_id serve a plain one)").c_str());
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, (f + ": between step_begin and step_finish (finish the step first)").c_str());
    return SPHX_OK;
}
// between the packing pass and the re-grid the local count is an upper bound and an advection may be pending: nothing is looked up then
int track_check_tile_state(sphx_ctx* c, const char* fn) {
    if (c->N && (!c->lists_current || c->tile_pending_dt > 0.0f))
        return c->fail(SPHX_ERR_NOT_READY, (std::string(fn) + ": the tile is between a halo exchange and its re-grid (sphx_sub_regrid first)").c_str());
    return SPHX_OK;
}

// found[] of the tile's owned particles, then per distinct id the slot word, {x, y, vx, vy} and the density
int track_tile_enqueue(sphx_ctx* c, uint4* o_frame, uint32_t* o_slot, uint32_t* o_density) {
    sphx_ctx::Track& t = c->track;
    hipStream_t st = c->stream;
    const uint32_t rev = c->K.rev;  // (launch() toggles the sweep direction of the step's next kernels: put back below)
    hipError_t he = hipMemsetAsync(t.found, 0, (size_t)t.unique * 4, st);
    if (he == hipSuccess) {
        const uint32_t n = c->N;
        if (n) {
            const TrackTable T{t.table, t.filter, t.found, t.unique, t.log2_bits};
            const uint32_t grid = std::min((n + TRACK_CHUNK - 1u) / TRACK_CHUNK, TRACK_MAX_GRID);
            const uint32_t lds = (1u << t.log2_bits) / 8u;
            launch(c, "track_lookup_owned", 4.0 * n, [&] {
                if (n >= TRACK_NT_FROM)
                    hipLaunchKernelGGL((k_track_lookup<true, true>), dim3(grid), dim3(256), lds, st, (const uint32_t*)c->pid, n, T);
                else
                    hipLaunchKernelGGL((k_track_lookup<false, true>), dim3(grid), dim3(256), lds, st, (const uint32_t*)c->pid, n, T);
            });
        }
        TrackEmit e = track_emit_args(c, t.found, nullptr, t.unique);
        e.o_frame = o_frame;
        e.o_slot = o_slot;
        e.o_density = o_density;
        track_enqueue_emit(c, e);
    }
    c->K.rev = rev;
    return he == hipSuccess ? SPHX_OK : c->fail(SPHX_ERR_HIP, "track_tile_enqueue: hipMemsetAsync", hipGetErrorString(he));
}

}  // namespace

extern "C" {

int sphx_tile_track_install(sphx_ctx* c, const uint32_t* table, const uint32_t* filter, uint32_t unique, uint32_t log2_bits) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (unique > TRACK_MAX_IDS) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_track_install: unique is larger than SPHX_TRACK_MAX_IDS");
    if (unique && (!table || !filter)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_track_install: table or filter is NULL with unique > 0");
    if (unique && (log2_bits < TRACK_FILTER_LOG2_MIN || log2_bits > TRACK_FILTER_LOG2_MAX))
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_track_install: log2_bits is outside the filter sizes of sphx_track_set.hpp");
    int rc;
    if ((rc = track_check_tile(c, "sphx_tile_track_install"))) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));  // (a queued frame or fetch may still read the old tables)
    sphx_ctx::Track& t = c->track;
    track_drop_recording(c);
    t.m = t.unique = 0;
    t.table = t.map = t.filter = t.found = nullptr;
    if (unique == 0) {
        dev_free(&t.set_buf);
        return SPHX_OK;
    }
    const size_t u = unique, fw = (size_t)1u << (log2_bits - 5u);
    if ((rc = dev_alloc(c, &t.set_buf, u + fw + u))) return rc;
    SPHX_HIP(c, hipMemcpyAsync(t.set_buf, table, u * 4, hipMemcpyHostToDevice, c->stream));
    SPHX_HIP(c, hipMemcpyAsync(t.set_buf + u, filter, fw * 4, hipMemcpyHostToDevice, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));  // (the host tables may go away with this call)
    t.table = t.set_buf;
    t.filter = t.table + u;
    t.found = t.filter + fw;
    t.m = t.unique = unique;
    t.log2_bits = log2_bits;
    return SPHX_OK;
}

// scratch of a fetch: [unique] {x, y, vx, vy} | [unique] slot words | [unique] densities
int sphx_tile_track_fetch_enqueue(sphx_ctx* c) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = track_check_tile(c, "sphx_tile_track_fetch_enqueue"))) return rc;
    if ((rc = track_check_tile_state(c, "sphx_tile_track_fetch_enqueue"))) return rc;
    sphx_ctx::Track& t = c->track;
    if (!t.unique) return SPHX_OK;
    SPHX_HIP(c, hipSetDevice(c->device));
    const size_t u = t.unique;
    if ((rc = track_scratch(c, 6 * u))) return rc;
    return track_tile_enqueue(c, (uint4*)t.scratch, t.scratch + 4 * u, t.scratch + 5 * u);
}

int sphx_tile_track_fetch(sphx_ctx* c, uint32_t* slot, float* xyvv, float* density) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!slot || !xyvv || !density) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_track_fetch: slot, xyvv or density is NULL");
    int rc;
    if ((rc = track_check_tile(c, "sphx_tile_track_fetch"))) return rc;
    sphx_ctx::Track& t = c->track;
    const size_t u = t.unique;
    if (!u) return SPHX_OK;
    if (t.scratch_cap < 6 * u) return c->fail(SPHX_ERR_NOT_READY, "sphx_tile_track_fetch: no sphx_tile_track_fetch_enqueue before it");
    SPHX_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    SPHX_HIP(c, hipMemcpyAsync(xyvv, t.scratch, u * 16, hipMemcpyDeviceToHost, st));
    SPHX_HIP(c, hipMemcpyAsync(slot, t.scratch + 4 * u, u * 4, hipMemcpyDeviceToHost, st));
    SPHX_HIP(c, hipMemcpyAsync(density, t.scratch + 5 * u, u * 4, hipMemcpyDeviceToHost, st));
    SPHX_HIP(c, hipStreamSynchronize(st));
    return SPHX_OK;
}

// scratch of a window: the counter (16 bytes: the records stay 16-byte aligned), then cap_records records of 32 bytes
int sphx_tile_track_window_enqueue(sphx_ctx* c, uint32_t first_id, uint32_t count, uint32_t cap_records) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (count > TRACK_WINDOW) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_track_window_enqueue: count is larger than the window of 2^22 ids");
    if (const char* bad = track_check_range(first_id, count)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_track_window_enqueue", bad);
    int rc;
    if ((rc = track_check_tile(c, "sphx_tile_track_window_enqueue"))) return rc;
    if ((rc = track_check_tile_state(c, "sphx_tile_track_window_enqueue"))) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    sphx_ctx::Track& t = c->track;
    const size_t words = sphx_track_host::HEADER_WORDS + (size_t)cap_records * sphx_track_host::RECORD_WORDS;
    if ((rc = track_scratch(c, words))) return rc;
    hipStream_t st = c->stream;
    SPHX_HIP(c, hipMemsetAsync(t.scratch, 0, sphx_track_host::HEADER_WORDS * 4, st));
    t.window_cap = cap_records;
    const uint32_t n = c->N;
    if (!n || !count) return SPHX_OK;
    const uint32_t rev = c->K.rev;
    const uint32_t grid = std::min((n + TRACK_CHUNK - 1u) / TRACK_CHUNK, TRACK_MAX_GRID);
    uint32_t* const head = t.scratch;
    uint4* const rec = (uint4*)(t.scratch + sphx_track_host::HEADER_WORDS);
    launch(c, "track_window_owned", 4.0 * n + 60.0 * std::min(cap_records, count), [&] {
        if (n >= TRACK_NT_FROM)
            hipLaunchKernelGGL(k_track_window_owned<true>, dim3(grid), dim3(256), 0, st, (const uint32_t*)c->pid, n, first_id, count, (const uint2*)c->posA,
                               (const uint2*)c->vel, (const uint32_t*)c->density, head, rec, cap_records);
        else
            hipLaunchKernelGGL(k_track_window_owned<false>, dim3(grid), dim3(256), 0, st, (const uint32_t*)c->pid, n, first_id, count, (const uint2*)c->posA,
                               (const uint2*)c->vel, (const uint32_t*)c->density, head, rec, cap_records);
    });
    c->K.rev = rev;
    return SPHX_OK;
}

int sphx_tile_track_window_fetch(sphx_ctx* c, uint32_t* records, uint32_t* out_n) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!records || !out_n) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_track_window_fetch: records or out_n is NULL");
    *out_n = 0;
    int rc;
    if ((rc = track_check_tile(c, "sphx_tile_track_window_fetch"))) return rc;
    sphx_ctx::Track& t = c->track;
    const size_t words = sphx_track_host::HEADER_WORDS + (size_t)t.window_cap * sphx_track_host::RECORD_WORDS;
    if (t.scratch_cap < words || !t.scratch) return c->fail(SPHX_ERR_NOT_READY, "sphx_tile_track_window_fetch: no sphx_tile_track_window_enqueue before it");
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipMemcpyAsync(records, t.scratch, words * 4, hipMemcpyDeviceToHost, c->stream));  // (counter and records in one transfer)
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    if (records[0] > t.window_cap) {
        *out_n = t.window_cap;
        return c->fail(SPHX_ERR_CAPACITY, "sphx_tile_track_window_fetch: the tile holds more owned particles of the window than cap_records (none was written past it)");
    }
    *out_n = records[0];
    return SPHX_OK;
}

// rec: [max_frames][unique] {x, y, vx, vy}, then [max_frames][unique] presence words (both regions 16-byte aligned for any unique)
int sphx_tile_track_record(sphx_ctx* c, uint32_t max_frames, uint32_t every) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = track_check_tile(c, "sphx_tile_track_record"))) return rc;
    sphx_ctx::Track& t = c->track;
    if (max_frames) {  // (max_frames == 0 stops and frees, whatever `every` says)
        if (every == 0) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_track_record: every is 0");
        if ((uint64_t)max_frames * t.unique * sphx_track_host::FRAME_ENTRY_BYTES > sphx_track_host::RECORD_MAX_BYTES)
            return c->fail(SPHX_ERR_CAPACITY, "sphx_tile_track_record: max_frames * unique * 20 bytes is more than 1 GiB");
        if (!t.unique) return c->fail(SPHX_ERR_NOT_READY, "sphx_tile_track_record: the tracked set is empty (sphx_tile_track_install first)");
    }
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));  // (a queued frame may still write the old buffer)
    track_drop_recording(c);
    if (!max_frames) return SPHX_OK;
    const size_t entries = (size_t)max_frames * t.unique;
    if ((rc = dev_alloc(c, &t.rec, entries * 5 + 4))) return rc;
    t.max_frames = max_frames;
    t.every = every;
    t.recording = 1u;
    return SPHX_OK;
}

// The tile loop calls this at the end of every finished step: with a recording on, every `every`-th call queues one frame of the owned
// particles behind the step's kernels.  Nothing comes back to the host and nothing is waited for.
int sphx_tile_track_frame(sphx_ctx* c) {
    if (!c || !c->tile_mode) return SPHX_ERR_INVALID_ARGUMENT;
    sphx_ctx::Track& t = c->track;
    if (!t.recording) return SPHX_OK;
    if (++t.steps % t.every) return SPHX_OK;
    if (t.frames >= t.max_frames) {
        t.dropped += 1u;
        return SPHX_OK;
    }
    int rc;
    if ((rc = track_check_tile_state(c, "sphx_tile_track_frame"))) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    const size_t u = t.unique, entries = (size_t)t.max_frames * u;
    uint32_t* const words = (uint32_t*)t.rec;
    if ((rc = track_tile_enqueue(c, (uint4*)words + (size_t)t.frames * u, words + 4 * entries + (size_t)t.frames * u, nullptr))) return rc;
    t.frames += 1u;
    return SPHX_OK;
}

int sphx_tile_track_read(sphx_ctx* c, uint32_t first_frame, uint32_t n_frames, float* xyvv, uint32_t* slot) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = track_check_tile(c, "sphx_tile_track_read"))) return rc;
    const sphx_ctx::Track& t = c->track;
    if ((uint64_t)first_frame + n_frames > t.frames)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_track_read: first_frame + n_frames is beyond the frames recorded (sphx_track_get_status)");
    if (n_frames == 0) return SPHX_OK;
    if (!xyvv || !slot) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_track_read: xyvv or slot is NULL");
    SPHX_HIP(c, hipSetDevice(c->device));
    const size_t u = t.unique, entries = (size_t)t.max_frames * u;
    const uint32_t* const words = (const uint32_t*)t.rec;
    SPHX_HIP(c, hipMemcpyAsync(xyvv, words + 4 * (size_t)first_frame * u, (size_t)n_frames * u * 16, hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipMemcpyAsync(slot, words + 4 * entries + (size_t)first_frame * u, (size_t)n_frames * u * 4, hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    return SPHX_OK;
}

}  // extern "C"
