// sphx_state.inc — a context saved into and restored from one blob (sphx_state_*, include/sphx.h; the layout and its validation are plain
// host code in sphx_state_format.hpp).  The one kernel here is the section digest; everything else is copies and host bookkeeping.
// Included at the end of sphx_kernels.hip (one translation unit: the launch layer of sphx_launch.inc is visible).
#include <cerrno>

#include "sphx_state_format.hpp"

namespace sphx {

// digest = sum_i (u64)w[i] * ((2 i + 1) * DIGEST_MUL) + W * DIGEST_LEN (mod 2^64), sphx.h.  The sum does not depend on the order of
// accumulation: every lane streams 16-byte pieces (word index 4 q .. 4 q + 3, so 2 i + 1 = 8 q + 1, + 2, + 2, + 2) into a 64-bit sum of
// its own, a wavefront folds its 64 sums with shuffles, the four wavefronts of a workgroup meet in LDS, and ONE atomic add whose result
// nobody reads leaves per workgroup.  `w` is 16-byte aligned (the library's own arrays); the W & 3 words behind the last whole piece and
// the length term are workgroup 0's.  *out is zeroed by the host before the launch.
__global__ __launch_bounds__(256) void k_state_digest(const uint32_t* __restrict__ w, unsigned long long W, unsigned long long* __restrict__ out) {
    constexpr unsigned long long M = sphx_state::DIGEST_MUL;
    __shared__ unsigned long long wave_sum[4];
    const uint4* __restrict__ v = (const uint4*)w;
    const unsigned long long n4 = W >> 2, stride = (unsigned long long)gridDim.x * 256ull;
    unsigned long long acc = 0;
#pragma unroll 4
    for (unsigned long long q = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; q < n4; q += stride) {
        const uint4 x = v[q];
        const unsigned long long k = (8ull * q + 1ull) * M;
        acc += (unsigned long long)x.x * k + (unsigned long long)x.y * (k + 2ull * M) + (unsigned long long)x.z * (k + 4ull * M) +
               (unsigned long long)x.w * (k + 6ull * M);
    }
    if (blockIdx.x == 0u && threadIdx.x < (uint32_t)(W & 3ull)) {
        const unsigned long long i = 4ull * n4 + threadIdx.x;  // (< W)
        acc += (unsigned long long)w[i] * ((2ull * i + 1ull) * M);
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) acc += __shfl_down(acc, off);
    if ((threadIdx.x & 63u) == 0u) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0u) {
        unsigned long long s = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        if (blockIdx.x == 0u) s += W * sphx_state::DIGEST_LEN;
        atomicAdd(out, s);  // (result unused: a non-returning 64-bit add)
    }
}

}  // namespace sphx

// ---- launch layer and C ABI ----------------------------------------------------------------------------------------------------------
namespace {

using sphx_state::Header;
constexpr uint32_t STATE_NSEC = sphx_state::NSEC;

// the refusals save, digest and load share (need_state: save and digest read a state that must exist)
int state_check(sphx_ctx* c, const char* fn, bool need_state) {
    const std::string f = fn;
    if (c->tile_mode)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, (f + ": not available on a tile context (its arrays hold ghosts and miss the particles other tiles own)").c_str());
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, (f + ": between step_begin and step_finish (finish the step first)").c_str());
    if (need_state && !c->uploaded) return c->fail(SPHX_ERR_NOT_READY, (f + ": the context holds no state (upload or load one first)").c_str());
    return SPHX_OK;
}

// the header of the live state: params, scalars and the layout they imply (digests not yet filled)
void state_header_of(const sphx_ctx* c, Header& h) {
    std::memset(&h, 0, sizeof(h));
    h.params = c->P;
    h.params.device = 0;
    h.s.n = c->N;
    h.s.b = c->B;
    h.s.cached_n = c->cached_n;
    h.s.wcsph_n = c->wcsph_n;
    h.s.ids_issued = c->ids_issued;
    h.s.num_density_iters = c->num_density_iters;
    h.s.num_divergence_iters = c->num_divergence_iters;
    h.s.set_changed = c->set_changed ? 1u : 0u;
    h.s.tiling_invariant = c->tiling_invariant ? 1u : 0u;
    // (a boundary replaced since the last build: the lists still hold neighbours of the old one, which the blob does not have)
    h.s.lists_current = c->lists_current && !c->boundary_changed ? 1u : 0u;
    h.s.sampling_allowed = c->sample_ready == 2u && h.s.lists_current ? 1u : 0u;
    sphx_state::layout(h);
}

// the device array behind section k of the live state (the boundary section lives on the host, in caller order: nullptr)
const void* state_section_ptr(const sphx_ctx* c, uint32_t k) {
    switch (k) {
        case SPHX_STATE_SEC_POSITIONS: return c->posA;
        case SPHX_STATE_SEC_VELOCITIES: return c->vel;
        case SPHX_STATE_SEC_PARTICLE_ID: return c->pid;
        case SPHX_STATE_SEC_DENSITY: return c->density;
        case SPHX_STATE_SEC_ALPHA: return c->alpha;
        case SPHX_STATE_SEC_KAPPA: return c->kappa;
        case SPHX_STATE_SEC_STIFFNESS: return c->stiff;
        case SPHX_STATE_SEC_ACCEL: return c->accel;
        default: return nullptr;
    }
}

// Digests of the device sections, by the layout of h, into dig[] (dig[boundary] from the host copy).  Synchronises the stream.
int state_digests(sphx_ctx* c, const Header& h, uint64_t* dig) {
    if (!c->state_dig) SPHX_HIP(c, hipMalloc((void**)&c->state_dig, STATE_NSEC * sizeof(unsigned long long)));
    // (the blob holds accel[] only for WCSPH: then a fill that a rigid non-pressure pass left out comes first, sphx::AccelUniform)
    if (h.sec[SPHX_STATE_SEC_ACCEL].bytes) read_accel(c);
    hipStream_t st = c->stream;
    SPHX_HIP(c, hipMemsetAsync(c->state_dig, 0, STATE_NSEC * sizeof(unsigned long long), st));
    for (uint32_t k = 0; k < STATE_NSEC; ++k) {
        const void* p = state_section_ptr(c, k);
        const unsigned long long W = h.sec[k].bytes / 4u;
        if (!p || !W) continue;  // (an empty section's digest is 0: the memset's)
        // memory-bound streaming pass: a workgroup per 256 pieces, capped at 2 048 workgroups (8 per CU) that stride over the rest
        const unsigned long long want = ((W >> 2) + 255ull) / 256ull;
        const uint32_t grid = (uint32_t)std::min<unsigned long long>(std::max<unsigned long long>(want, 1ull), 2048ull);
        hipLaunchKernelGGL(k_state_digest, dim3(grid), dim3(256), 0, st, (const uint32_t*)p, W, c->state_dig + k);
    }
    unsigned long long host[STATE_NSEC];
    SPHX_HIP(c, hipMemcpyAsync(host, c->state_dig, sizeof(host), hipMemcpyDeviceToHost, st));
    SPHX_HIP(c, hipStreamSynchronize(st));
    for (uint32_t k = 0; k < STATE_NSEC; ++k) dig[k] = host[k];
    dig[SPHX_STATE_SEC_BOUNDARY] = sphx_state::digest_words(c->h_boundary.data(), h.sec[SPHX_STATE_SEC_BOUNDARY].bytes / 4u);
    return SPHX_OK;
}

}  // namespace

extern "C" {

int sphx_state_size(sphx_ctx* c, uint64_t* out_bytes) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!out_bytes) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_state_size: out_bytes is NULL");
    *out_bytes = 0;
    if (int rc = state_check(c, "sphx_state_size", true)) return rc;
    Header h;
    state_header_of(c, h);
    *out_bytes = h.total_bytes;
    return SPHX_OK;
}

int sphx_state_digest(sphx_ctx* c, uint64_t* out) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_state_digest: out is NULL");
    if (int rc = state_check(c, "sphx_state_digest", true)) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    Header h;
    state_header_of(c, h);
    return state_digests(c, h, out);
}

int sphx_state_save(sphx_ctx* c, void* buf, uint64_t capacity, uint32_t flags, uint64_t* out_bytes) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (out_bytes) *out_bytes = 0;
    if (flags & ~(uint32_t)SPHX_STATE_DEVICE_BUFFER) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_state_save: unknown flags bits");
    if (int rc = state_check(c, "sphx_state_save", true)) return rc;
    Header h;
    state_header_of(c, h);
    if (out_bytes) *out_bytes = h.total_bytes;
    if (!buf) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_state_save: buf is NULL");
    if (capacity < h.total_bytes) return c->fail(SPHX_ERR_CAPACITY, "sphx_state_save: the buffer is smaller than sphx_state_size");
    SPHX_HIP(c, hipSetDevice(c->device));
    uint64_t dig[STATE_NSEC];
    if (int rc = state_digests(c, h, dig)) return rc;
    for (uint32_t k = 0; k < STATE_NSEC; ++k) h.sec[k].digest = dig[k];
    sphx_state::seal(h);
    const bool dev = (flags & SPHX_STATE_DEVICE_BUFFER) != 0;
    unsigned char* const b = (unsigned char*)buf;
    hipStream_t st = c->stream;
    if (dev)
        SPHX_HIP(c, hipMemcpyAsync(b, &h, sizeof(h), hipMemcpyHostToDevice, st));
    else
        std::memcpy(b, &h, sizeof(h));
    for (uint32_t k = 0; k < STATE_NSEC; ++k) {
        const uint64_t off = h.sec[k].offset, bytes = h.sec[k].bytes, next = k + 1 < STATE_NSEC ? h.sec[k + 1].offset : h.total_bytes;
        const void* p = state_section_ptr(c, k);
        if (bytes) {
            if (p)
                SPHX_HIP(c, hipMemcpyAsync(b + off, p, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
            else if (dev)
                SPHX_HIP(c, hipMemcpyAsync(b + off, c->h_boundary.data(), bytes, hipMemcpyHostToDevice, st));
            else
                std::memcpy(b + off, c->h_boundary.data(), bytes);
        }
        if (const uint64_t pad = next - (off + bytes)) {  // (0 or 4 bytes)
            if (dev)
                SPHX_HIP(c, hipMemsetAsync(b + off + bytes, 0, pad, st));
            else
                std::memset(b + off + bytes, 0, pad);
        }
    }
    SPHX_HIP(c, hipStreamSynchronize(st));
    return SPHX_OK;
}

int sphx_state_load(sphx_ctx* c, const void* buf, uint64_t bytes, uint32_t flags) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (flags & ~(uint32_t)SPHX_STATE_DEVICE_BUFFER) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_state_load: unknown flags bits");
    if (!buf) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_state_load: buf is NULL");
    if (int rc = state_check(c, "sphx_state_load", false)) return rc;
    const bool dev = (flags & SPHX_STATE_DEVICE_BUFFER) != 0;
    const unsigned char* const b = (const unsigned char*)buf;
    hipStream_t st = c->stream;
    // ---- host-side validation: nothing of the context changes before it has passed ------------------------------------------------------
    if (bytes < sphx_state::HEADER_BYTES) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_state_load", "truncated: shorter than the header");
    unsigned char head[sphx_state::HEADER_BYTES];
    if (dev) {
        SPHX_HIP(c, hipSetDevice(c->device));
        SPHX_HIP(c, hipMemcpyAsync(head, b, sizeof(head), hipMemcpyDeviceToHost, st));
        SPHX_HIP(c, hipStreamSynchronize(st));
    } else {
        std::memcpy(head, b, sizeof(head));
    }
    Header h;
    std::string why;
    if (!sphx_state::validate(head, bytes, &h, &why)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_state_load", why.c_str());
    if (const char* field = sphx_state::params_mismatch(h.params, c->P))
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_state_load: the blob was saved under other params than this context's; first field that differs", field);
    if ((h.s.tiling_invariant != 0) != c->tiling_invariant)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, h.s.tiling_invariant ? "sphx_state_load: the blob was saved in tiling-invariant mode, this context is not in it"
                                                                       : "sphx_state_load: this context is in tiling-invariant mode, the blob was not saved in it");
    const uint32_t n = h.s.n, nb = h.s.b;
    // the host needs the positions (the covered region is derived from them, as in sphx_upload) and the boundary (its caller order)
    std::vector<float> hpos((size_t)n * 2), hbnd((size_t)nb * 2);
    const sphx_state::Section &sp = h.sec[SPHX_STATE_SEC_POSITIONS], &sb = h.sec[SPHX_STATE_SEC_BOUNDARY];
    if (dev) {
        if (sp.bytes) SPHX_HIP(c, hipMemcpyAsync(hpos.data(), b + sp.offset, sp.bytes, hipMemcpyDeviceToHost, st));
        if (sb.bytes) SPHX_HIP(c, hipMemcpyAsync(hbnd.data(), b + sb.offset, sb.bytes, hipMemcpyDeviceToHost, st));
        SPHX_HIP(c, hipStreamSynchronize(st));
    } else {
        if (sp.bytes) std::memcpy(hpos.data(), b + sp.offset, sp.bytes);
        if (sb.bytes) std::memcpy(hbnd.data(), b + sb.offset, sb.bytes);
    }
    if (sphx_state::digest_words(hbnd.data(), sb.bytes / 4u) != sb.digest)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_state_load: digest mismatch in section", sphx_state::section_name(SPHX_STATE_SEC_BOUNDARY));
    // ---- from here on the context changes ---------------------------------------------------------------------------------------------------
    SPHX_HIP(c, hipSetDevice(c->device));
    c->ahead.valid = false;  // a queued run-ahead pass read the state that is being replaced
    auto broken = [&](int code) {  // the context holds half a state: it asks for an upload or a load, as after a failed step
        c->uploaded = false;
        return code;
    };
    int rc;
    // the boundary, through the one path that installs one (a rollback inside one context keeps the boundary and its grid)
    if (hbnd.size() != c->h_boundary.size() || (nb && std::memcmp(hbnd.data(), c->h_boundary.data(), hbnd.size() * 4) != 0)) {
        if ((rc = sphx_set_boundary(c, nb ? hbnd.data() : nullptr, nb))) return broken(rc);
    }
    sample_went_stale(c, "sphx_state_load did not complete: upload or load the state again");
    SPHX_HIP(c, hipStreamSynchronize(st));
    clear_histograms(c);
    if ((rc = alloc_particles(c, std::max(n, h.s.wcsph_n)))) return broken(rc);
    c->N = n;
    lists_went_stale(c);
    // (accelerations about to arrive replace what a rigid non-pressure pass owes the array: paid now, not over them by the digest below)
    if (h.sec[SPHX_STATE_SEC_ACCEL].bytes) read_accel(c);
    if (c->capN) {  // the slot-bound slots the blob does not hold read zero
        SPHX_HIP(c, hipMemsetAsync(c->alpha, 0, (size_t)c->capN * 4, st));
        SPHX_HIP(c, hipMemsetAsync(c->kappa, 0, (size_t)c->capN * 4, st));
        SPHX_HIP(c, hipMemsetAsync(c->stiff, 0, (size_t)c->capN * 4, st));
    }
    for (uint32_t k = 0; k < STATE_NSEC; ++k) {
        void* p = const_cast<void*>(state_section_ptr(c, k));
        if (p && h.sec[k].bytes)  // (bytes <= 8 * max(n, wcsph_n) <= 8 * capN: inside the array)
            SPHX_HIP(c, hipMemcpyAsync(p, b + h.sec[k].offset, h.sec[k].bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    }
    // what arrived, digested where it now lives (the boundary's digest was checked above, on the host copy that is now h_boundary)
    uint64_t dig[STATE_NSEC];
    if ((rc = state_digests(c, h, dig))) return broken(rc);
    for (uint32_t k = 0; k < STATE_NSEC; ++k)
        if (dig[k] != h.sec[k].digest)
            return broken(c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_state_load: digest mismatch in section (upload or load the state again)", sphx_state::section_name(k)));
    c->cached_n = h.s.cached_n;
    c->wcsph_n = h.s.wcsph_n;
    c->ids_issued = h.s.ids_issued;
    c->num_density_iters = h.s.num_density_iters;
    c->num_divergence_iters = h.s.num_divergence_iters;
    c->set_changed = h.s.set_changed != 0;
    c->in_wcsph = false;
    c->handoff.clear();
    c->need_expand = c->need_recover = false;  // (they described the particles that were here before)
    c->recover_streak = c->recover_cooldown = 0;
    c->uploaded = true;
    // the covered region, as sphx_upload derives it
    c->have_fluid_bbox = cell_bbox(c, hpos.data(), n, c->fb);
    c->gdyn.cover.clear();
    c->gdyn.nbx = c->gdyn.nby = 0;
    if (c->have_fluid_bbox && (rc = cover_dynamic(c, hpos.data(), n, false))) return broken(rc);
    if ((rc = ensure_index_scratch(c))) return broken(rc);
    if (h.s.lists_current) {
        // one neighbour build, not a step: no density, no alpha, no SPHX_FLAG_*; the re-grid of a sorted set is the identity
        const uint32_t flags_before = c->step_flags;
        if ((rc = update_neighborhood(c, false, 0.0f, false)) || (rc = publish_and_wait(c))) return broken(rc);
        c->step_flags = flags_before;
        if (h.s.sampling_allowed) c->sample_ready = 2u;
    } else {
        // nobody can restore stale lists: where the next step would have walked them (dfsph.rs:419 sees the cached count), it re-grids
        if (c->cached_n == n && n) c->set_changed = true;
        sample_went_stale(c, "the loaded state held no current neighbour lists: run a step, or sphx_update_neighborhood + sphx_update_densities");
    }
    return SPHX_OK;
}

int sphx_state_save_file(sphx_ctx* c, const char* path) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!path) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_state_save_file: path is NULL");
    uint64_t bytes = 0;
    int rc;
    if ((rc = sphx_state_size(c, &bytes))) return rc;
    std::vector<unsigned char> blob(bytes);
    if ((rc = sphx_state_save(c, blob.data(), bytes, 0u, nullptr))) return rc;
    const std::string tmp = std::string(path) + ".tmp";
    FILE* f = std::fopen(tmp.c_str(), "wb");
    bool ok = f != nullptr;
    if (ok) {
        ok = std::fwrite(blob.data(), 1, blob.size(), f) == blob.size();
        ok = std::fclose(f) == 0 && ok;
    }
    if (ok) ok = std::rename(tmp.c_str(), path) == 0;
    if (!ok) {
        const std::string e = std::strerror(errno);
        std::remove(tmp.c_str());
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_state_save_file: cannot write the file", e.c_str());
    }
    return SPHX_OK;
}

int sphx_state_load_file(sphx_ctx* c, const char* path) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!path) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_state_load_file: path is NULL");
    FILE* f = std::fopen(path, "rb");
    if (!f) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_state_load_file: cannot open the file", std::strerror(errno));
    std::vector<unsigned char> blob;
    unsigned char chunk[1 << 16];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) blob.insert(blob.end(), chunk, chunk + got);
    const bool bad = std::ferror(f) != 0;
    std::fclose(f);
    if (bad) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_state_load_file: cannot read the file");
    return sphx_state_load(c, blob.empty() ? (const void*)"" : (const void*)blob.data(), blob.size(), 0u);
}

}  // extern "C"
