// sphx_multi_state.inc — the device half of a tiled run's checkpoint (sphx_multi_state_*, include/sphx.h; the host half is in
// sphx_tiles.cpp, the part's layout in sphx_multi_state_format.hpp): the particles a tile OWNS, compacted in local device order into
// seven contiguous section buffers, with an id-keyed digest per section accumulated on the way.
// Included at the end of sphx_kernels.hip (one translation unit: the launch layer of sphx_launch.inc and k_remove_scan are visible).
#include "sphx_multi_state_format.hpp"

namespace sphx {

struct MStateOut {
    float2 *pos, *vel;
    uint32_t* id;
    float *density, *alpha, *kappa, *stiff;
};

// Stable compaction as in sphx_edit.inc (DESIGN.md §4e): owned particles per 256-particle piece, their exclusive scan (k_remove_scan),
// then the move.  Pieces are numbered by their place in the arrays, not by the workgroup that happens to run them: no atomic decides a
// slot.  pass 1: owned particles (bit 31 of the id) per piece
__global__ __launch_bounds__(256) void k_mstate_count(const uint32_t* __restrict__ pid, uint32_t n, uint32_t* __restrict__ wg_owned) {
    __shared__ uint32_t wave_owned[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool own = i < n && (pid[i] >> 31);
    const unsigned long long m = __ballot(own);
    if ((threadIdx.x & 63u) == 0u) wave_owned[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0u) wg_owned[blockIdx.x] = wave_owned[0] + wave_owned[1] + wave_owned[2] + wave_owned[3];
}

// pass 3: the streaming pass.  A workgroup takes the pieces blockIdx.x, blockIdx.x + gridDim.x, ... (at most 2 048 workgroups); an owned
// particle goes to slot = piece offset + owned particles of the wavefronts before this one (LDS) + rank among the wavefront's owned
// (ballot + mbcnt) — inside [0, n_owned), and n_owned <= n, the capacity of every section buffer.  36 bytes read per local particle,
// 36 written per owned one.  Digest (sphx.h): the word c of a section with k words per particle has the index id * k + c, so
// its multiplier is (2 (id k + c) + 1) M: (4 id + 1) M and (4 id + 3) M for the two words of a position or velocity, (2 id + 1) M for
// the others.  Integer sums mod 2^64: every lane keeps seven of its own over all its pieces, a wavefront folds them with shuffles, the
// four wavefronts meet in LDS, and seven atomic adds whose result nobody reads leave per workgroup.  zero_mask bit 0 / 1: kappa /
// stiffness are written (and digested) as +0.0 — the next solver loop zeroes them before it reads them.
__global__ __launch_bounds__(256) void k_mstate_pack(const float2* __restrict__ pos, const float2* __restrict__ vel, const uint32_t* __restrict__ pid,
                                                     const float* __restrict__ density, const float* __restrict__ alpha, const float* __restrict__ kappa,
                                                     const float* __restrict__ stiff, uint32_t n, uint32_t nb, const uint32_t* __restrict__ wg_off,
                                                     uint32_t zero_mask, MStateOut o, unsigned long long* __restrict__ dig) {
    constexpr unsigned long long M = sphx_multi_state::DIGEST_MUL;
    __shared__ uint32_t wave_owned[4];
    __shared__ unsigned long long wave_sum[4][7];
    unsigned long long acc[7] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    const uint32_t w = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x; t < nb; t += gridDim.x) {  // (t is the same for the whole workgroup: the barriers are uniform)
        const uint32_t i = t * 256u + threadIdx.x;
        const uint32_t raw = i < n ? pid[i] : 0u;
        const bool own = (raw >> 31) != 0u;
        const unsigned long long m = __ballot(own);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if ((threadIdx.x & 63u) == 0u) wave_owned[w] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t base = wg_off[t];
#pragma unroll
        for (uint32_t k = 0; k < 3u; ++k) base += k < w ? wave_owned[k] : 0u;
        __syncthreads();  // (the next piece overwrites wave_owned)
        if (own) {
            const uint32_t d = base + rank, id = raw & 0x7FFFFFFFu;
            const float2 p = pos[i], v = vel[i];
            const float rho = density[i], a = alpha[i];
            const float ka = (zero_mask & 1u) ? 0.0f : kappa[i], st = (zero_mask & 2u) ? 0.0f : stiff[i];
            o.pos[d] = p;
            o.vel[d] = v;
            o.id[d] = id;
            o.density[d] = rho;
            o.alpha[d] = a;
            o.kappa[d] = ka;
            o.stiff[d] = st;
            const unsigned long long m1 = (2ull * id + 1ull) * M, m2 = (4ull * id + 1ull) * M;
            acc[0] += (unsigned long long)__float_as_uint(p.x) * m2 + (unsigned long long)__float_as_uint(p.y) * (m2 + 2ull * M);
            acc[1] += (unsigned long long)__float_as_uint(v.x) * m2 + (unsigned long long)__float_as_uint(v.y) * (m2 + 2ull * M);
            acc[2] += (unsigned long long)id * m1;
            acc[3] += (unsigned long long)__float_as_uint(rho) * m1;
            acc[4] += (unsigned long long)__float_as_uint(a) * m1;
            acc[5] += (unsigned long long)__float_as_uint(ka) * m1;
            acc[6] += (unsigned long long)__float_as_uint(st) * m1;
        }
    }
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        unsigned long long x = acc[s];
#pragma unroll
        for (int off = 32; off; off >>= 1) x += __shfl_down(x, off);
        if ((threadIdx.x & 63u) == 0u) wave_sum[w][s] = x;
    }
    __syncthreads();
    if (threadIdx.x < 7u) {
        const uint32_t s = threadIdx.x;
        unsigned long long x = wave_sum[0][s] + wave_sum[1][s] + wave_sum[2][s] + wave_sum[3][s];
        // the length term: (n_owned k) * DIGEST_LEN, once (wg_off[nb] is the scan's total)
        if (blockIdx.x == 0u) x += (unsigned long long)wg_off[nb] * (s < 2u ? 2ull : 1ull) * sphx_multi_state::DIGEST_LEN;
        atomicAdd(dig + s, x);  // (result unused: a non-returning 64-bit add)
    }
}

}  // namespace sphx

// ---- launch layer and the internal seam of the tile loop ---------------------------------------------------------------------------------
namespace {

// the scratch of the pass, in 4-byte words: 16 (seven digests + one spare, 8 bytes each) | pos 2n | vel 2n | id, density, alpha, kappa,
// stiffness n each | owned per piece, then their scan, nb + 1
constexpr size_t MSTATE_DIG_WORDS = 16;
size_t mstate_words(uint32_t n) { return MSTATE_DIG_WORDS + 9ull * n + nblocks(n) + 1u; }
sphx::MStateOut mstate_sections(uint32_t* buf, uint32_t n) {
    uint32_t* p = buf + MSTATE_DIG_WORDS;
    sphx::MStateOut o;
    o.pos = (float2*)p;
    o.vel = (float2*)(p + 2ull * n);
    o.id = p + 4ull * n;
    o.density = (float*)(p + 5ull * n);
    o.alpha = (float*)(p + 6ull * n);
    o.kappa = (float*)(p + 7ull * n);
    o.stiff = (float*)(p + 8ull * n);
    return o;
}

}  // namespace

extern "C" {

int sphx_tile_state_pack(sphx_ctx* c, uint32_t flags, sphx_tile_state_out* out, uint64_t* out_digests, uint32_t* out_n_owned) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_state_pack: out is NULL");
    if (flags & ~(uint32_t)(SPHX_TILE_STATE_ZERO_KAPPA | SPHX_TILE_STATE_ZERO_STIFFNESS)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_tile_state_pack: unknown flags bits");
    int rc;
    if ((rc = stats_check_tile(c, "sphx_tile_state_pack"))) return rc;
    if ((rc = stats_check_tile_state(c, "sphx_tile_state_pack"))) return rc;
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t n = c->N, nb = nblocks(n);
    hipStream_t st = c->stream;
    const size_t need = mstate_words(n);
    if (need > c->mstate_cap) {
        SPHX_HIP(c, hipStreamSynchronize(st));  // (a queued pass may still write the old buffer)
        c->mstate_cap = 0;
        if ((rc = dev_alloc(c, &c->mstate_buf, need))) return rc;
        c->mstate_cap = need;
    }
    uint32_t* const buf = c->mstate_buf;
    uint32_t* const wg = buf + MSTATE_DIG_WORDS + 9ull * n;
    const sphx::MStateOut o = mstate_sections(buf, n);
    SPHX_HIP(c, hipMemsetAsync(buf, 0, MSTATE_DIG_WORDS * 4, st));
    const uint32_t rev = c->K.rev;  // (a checkpoint must not change the sweep direction of the step's next kernels: launch() toggles it)
    if (n) {
        launch(c, "mstate_count", 4.0 * n + 4.0 * nb, [&] { hipLaunchKernelGGL(sphx::k_mstate_count, dim3(nb), dim3(256), 0, st, (const uint32_t*)c->pid, n, wg); });
        launch(c, "mstate_scan", 8.0 * nb + 4.0, [&] { hipLaunchKernelGGL(sphx::k_remove_scan, dim3(1), dim3(256), 0, st, wg, nb); });
        launch(c, "mstate_pack", 36.0 * n + 4.0 * nb, [&] {
            hipLaunchKernelGGL(sphx::k_mstate_pack, dim3(std::min(nb, 2048u)), dim3(256), 0, st, (const float2*)c->posA, (const float2*)c->vel, (const uint32_t*)c->pid,
                               (const float*)c->density, (const float*)c->alpha, (const float*)c->kappa, (const float*)c->stiff, n, nb, (const uint32_t*)wg, flags, o,
                               (unsigned long long*)buf);
        });
    } else {
        SPHX_HIP(c, hipMemsetAsync(wg, 0, 4, st));  // (the total the fetch reads)
    }
    c->K.rev = rev;
    c->mstate_n = n;
    out->pos = (const float*)o.pos;
    out->vel = (const float*)o.vel;
    out->id = o.id;
    out->density = o.density;
    out->alpha = o.alpha;
    out->kappa = o.kappa;
    out->stiffness = o.stiff;
    if (out_digests || out_n_owned) return sphx_tile_state_fetch(c, out_digests, out_n_owned);
    return SPHX_OK;
}

int sphx_tile_state_fetch(sphx_ctx* c, uint64_t* out_digests, uint32_t* out_n_owned) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!c->mstate_buf) return c->fail(SPHX_ERR_NOT_READY, "sphx_tile_state_fetch: no sphx_tile_state_pack before it");
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t n = c->mstate_n;
    unsigned long long dig[7];
    uint32_t owned = 0;
    SPHX_HIP(c, hipMemcpyAsync(dig, c->mstate_buf, sizeof(dig), hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipMemcpyAsync(&owned, c->mstate_buf + MSTATE_DIG_WORDS + 9ull * n + nblocks(n), 4, hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    if (owned > n) return c->fail(SPHX_ERR_HIP, "sphx_tile_state_fetch: the owned count is larger than the local count");
    if (out_digests)
        for (int k = 0; k < 7; ++k) out_digests[k] = dig[k];
    if (out_n_owned) *out_n_owned = owned;
    return SPHX_OK;
}

int sphx_tile_upload_state(sphx_ctx* c, const float* pos_xy, const float* vel_xy, const uint32_t* ids, const float* kappa, const float* stiffness, uint32_t n) {
    int rc = sphx_tile_upload(c, pos_xy, vel_xy, ids, n);
    if (rc || !n) return rc;
    hipStream_t st = c->stream;
    // (n <= capN: sphx_upload has allocated for n)
    if (kappa)
        SPHX_HIP(c, hipMemcpyAsync(c->kappa, kappa, (size_t)n * 4, hipMemcpyHostToDevice, st));
    else
        SPHX_HIP(c, hipMemsetAsync(c->kappa, 0, (size_t)n * 4, st));
    if (stiffness)
        SPHX_HIP(c, hipMemcpyAsync(c->stiff, stiffness, (size_t)n * 4, hipMemcpyHostToDevice, st));
    else
        SPHX_HIP(c, hipMemsetAsync(c->stiff, 0, (size_t)n * 4, st));
    SPHX_HIP(c, hipStreamSynchronize(st));  // (the caller's arrays are borrowed for the duration of the call)
    return SPHX_OK;
}

int sphx_get_tiling_invariant(const sphx_ctx* c) { return c && c->tiling_invariant ? 1 : 0; }

}  // extern "C"
