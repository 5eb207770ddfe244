// sphx_fields.inc — per-particle flow fields (sphx_particle_fields, include/sphx.h): the velocity gradient with its divergence and
// vorticity, and the gradient of the colour field, from ONE traversal of the solver's own neighbour lists.  Included at the end of
// sphx_kernels.hip (one translation unit: nb_head, nb_stage, nb_traverse, Stage, wendland_grad and the launch layer of sphx_launch.inc
// are visible).  Compiled with -ffp-contract=off like the rest: the fp32 expressions below are the contract of sphx.h, restated bit for
// bit by tests/fields_reference.py.  Everything here only READS the particle state (DESIGN.md §4h).

namespace sphx {

struct FieldsArgs {
    float* vel_grad;    // [4n] or null
    float* divergence;  // [n] or null
    float* vorticity;   // [n] or null
    float* color_grad;  // [2n] or null
};

// The walk of k_nonpressure over ALL count_total entries (dynamic, then static), with the neighbour's VOLUME as the staged scalar:
// m / density[g] for a fluid record, m / rho0 for a boundary record (density[] has no boundary tail), formed once where the record
// is staged.  The boundary tail of vel[] is zero (k_fill_tails; no kernel writes it), so v_b = (0, 0) needs no select.
// VEL: the four sums of the velocity gradient (vel_grad, divergence, vorticity); COL: the two of the colour gradient.  A colour-only
// launch stages positions and volumes only (Stage<1, 1>, 12 KiB).  An accumulator's arithmetic is the same in every instantiation.
//
// OWNED (sphx_multi_particle_fields: one tile of a tiled run, whose arrays interleave owned particles and ghosts in Morton order): only a
// particle the tile owns (bit 31 of its id word) is answered, at its place among the owned ones — the order of sphx_multi_download.  The
// staging area fills the LDS budget of 8 workgroups per CU exactly (DESIGN.md §4h), so the slot costs no LDS: k_fields_count has left the
// owned count of every wavefront (run of 64 slots, numbered by its place in the arrays) and of every 256-slot piece, k_remove_scan the
// pieces' exclusive prefix; slot = piece offset + counts of the wavefronts before this one (scalar loads) + rank among the wavefront's
// owned lanes (ballot + mbcnt).  No atomic decides a slot.  A piece without an owned particle returns before the head's loads (a scalar
// test: whole stretches of a tile's Morton order are ghost band).  A ghost in a live piece takes full part in the staging — the other
// lanes' lists point at its slots — then walks nothing (lim = 0: nb_traverse masks by lim, __any skips a wavefront of ghosts) and stores
// nothing: a ghost's list is not complete.
struct FieldsOwned {
    const uint32_t* pid;       // [n] id words: bit 31 = owned by this tile
    const uint32_t* wave_cnt;  // [4 * pieces] owned lanes per wavefront
    const uint32_t* wg_off;    // [pieces + 1] exclusive prefix of the owned lanes per piece; [pieces] = the total
    uint32_t* ids;             // [n_owned] or null: id of entry k (31 bits)
};

template <bool VEL, bool COL>
__global__ NONP_BOUNDS void k_particle_fields(PVr PV, const float* __restrict__ density, uint32_t n, uint32_t soff, Consts K, NbView nb, FieldsArgs o) {
#define SPHX_FIELDS_OWNED 0
#include "sphx_fields_body.inc"
#undef SPHX_FIELDS_OWNED
}
template <bool VEL, bool COL>
__global__ NONP_BOUNDS void k_particle_fields_owned(PVr PV, const float* __restrict__ density, uint32_t n, uint32_t soff, Consts K, NbView nb, FieldsArgs o,
                                                    FieldsOwned w) {
#define SPHX_FIELDS_OWNED 1
#include "sphx_fields_body.inc"
#undef SPHX_FIELDS_OWNED
}

// the counting pass of the owned form: owned lanes per wavefront and per 256-slot piece, numbered by their place in the arrays
// (blockIdx.x, not xcd_bid(): the numbering must not depend on who runs a piece).  Pieces past the last particle count zero.
__global__ __launch_bounds__(256) void k_fields_count(const uint32_t* __restrict__ pid, uint32_t n, uint32_t* __restrict__ wave_cnt, uint32_t* __restrict__ wg_cnt) {
    __shared__ uint32_t wave_owned[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool own = i < n && (pid[i] >> 31);
    const uint32_t k = (uint32_t)__popcll(__ballot(own));
    if ((threadIdx.x & 63u) == 0u) {
        wave_owned[threadIdx.x >> 6] = k;
        wave_cnt[i >> 6] = k;
    }
    __syncthreads();
    if (threadIdx.x == 0u) wg_cnt[blockIdx.x] = wave_owned[0] + wave_owned[1] + wave_owned[2] + wave_owned[3];
}

}  // namespace sphx

// ---- launch layer and C ABI ----------------------------------------------------------------------------------------------------------
namespace {

// the traversal behind what is on the stream; the sweep direction launch() toggles is put back (as a sampling query does)
void enqueue_fields(sphx_ctx* c, const sphx_fields_out& out) {
    const uint32_t n = c->N;
    const bool vel = out.vel_grad || out.divergence || out.vorticity, col = out.color_grad != nullptr;
    const FieldsArgs a{out.vel_grad, out.divergence, out.vorticity, out.color_grad};
    const double bytes = (8.0 + (vel ? 8 : 0) + 4 + list_bytes(c) + (out.vel_grad ? 16 : 0) + (out.divergence ? 4 : 0) + (out.vorticity ? 4 : 0) + (col ? 8 : 0)) * n;
    const uint32_t rev = c->K.rev;
    hipStream_t st = c->stream;
    const dim3 g(nblocks(n)), b(256);
    launch(c, "particle_fields", bytes, [&] {
        if (vel && col)
            hipLaunchKernelGGL((k_particle_fields<true, true>), g, b, 0, st, c->pv(), (const float*)c->density, n, c->soff(), c->K, c->nbv(), a);
        else if (vel)
            hipLaunchKernelGGL((k_particle_fields<true, false>), g, b, 0, st, c->pv(), (const float*)c->density, n, c->soff(), c->K, c->nbv(), a);
        else
            hipLaunchKernelGGL((k_particle_fields<false, true>), g, b, 0, st, c->pv(), (const float*)c->density, n, c->soff(), c->K, c->nbv(), a);
    });
    c->K.rev = rev;
}

}  // namespace

extern "C" {

int sphx_particle_fields(sphx_ctx* c, uint32_t flags, const sphx_fields_out* out) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!out) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_particle_fields: out is NULL");
    if (!out->vel_grad && !out->divergence && !out->vorticity && !out->color_grad)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_particle_fields: out requests no output (every pointer is NULL)");
    if (flags & ~(uint32_t)SPHX_FIELDS_DEVICE_POINTERS) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_particle_fields: unknown flags bits");
    if (c->tile_mode)
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_particle_fields: not available on a tile context (its arrays hold ghosts and miss the particles other tiles own): "
                       "sphx_multi_particle_fields answers for the tiled run");
    int rc;
    if ((rc = sample_check_state(c, "sphx_particle_fields"))) return rc;
    // (sample_ready == 2 implies a completed build of these positions: lists_went_stale drops both together)
    if (!c->lists_current) return c->fail(SPHX_ERR_NOT_READY, "sphx_particle_fields: the neighbour lists do not belong to the current positions");
    const size_t n = c->N;
    if (n == 0) return SPHX_OK;
    SPHX_HIP(c, hipSetDevice(c->device));
    if (flags & SPHX_FIELDS_DEVICE_POINTERS) {
        enqueue_fields(c, *out);
        return SPHX_OK;
    }
    // host pointers: the walk writes device copies in the context's scratch (grown on demand for the requested outputs, freed in
    // sphx_destroy), the outputs come back before the return
    const size_t n_g = out->vel_grad ? 4 * n : 0, n_d = out->divergence ? n : 0, n_w = out->vorticity ? n : 0, n_c = out->color_grad ? 2 * n : 0;
    const size_t need = n_g + n_d + n_w + n_c;  // 4-byte words
    if (need > c->fields_cap) {
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
        if ((rc = dev_alloc(c, &c->fields_buf, need))) {
            c->fields_cap = 0;
            return rc;
        }
        c->fields_cap = need;
    }
    float* p = c->fields_buf;
    sphx_fields_out dev{};
    dev.vel_grad = out->vel_grad ? p : nullptr;
    p += n_g;
    dev.divergence = out->divergence ? p : nullptr;
    p += n_d;
    dev.vorticity = out->vorticity ? p : nullptr;
    p += n_w;
    dev.color_grad = out->color_grad ? p : nullptr;
    enqueue_fields(c, dev);
    hipStream_t st = c->stream;
    if (n_g) SPHX_HIP(c, hipMemcpyAsync(out->vel_grad, dev.vel_grad, n_g * 4, hipMemcpyDeviceToHost, st));
    if (n_d) SPHX_HIP(c, hipMemcpyAsync(out->divergence, dev.divergence, n_d * 4, hipMemcpyDeviceToHost, st));
    if (n_w) SPHX_HIP(c, hipMemcpyAsync(out->vorticity, dev.vorticity, n_w * 4, hipMemcpyDeviceToHost, st));
    if (n_c) SPHX_HIP(c, hipMemcpyAsync(out->color_grad, dev.color_grad, n_c * 4, hipMemcpyDeviceToHost, st));
    SPHX_HIP(c, hipStreamSynchronize(st));
    return SPHX_OK;
}

}  // extern "C"

// ---- one tile of a tiled run: the seam sphx_multi_particle_fields (sphx_tiles.cpp) is built on -------------------------------------------
// Enqueue and fetch halves, like the sampling seam: the multi enqueues on every tile's stream first and then collects, so the tiles'
// passes overlap.  The scratch is fields_buf (sphx_particle_fields refuses a tile context, so nobody else uses it there), in 4-byte
// words: owned lanes per wavefront [4 nb] | per piece, then their exclusive prefix [nb + 1, padded to a multiple of 4] | ids [n, padded
// to even] | the requested outputs for n entries each (n = local count, an upper bound of the owned count: the walk can be queued
// before that count is known on the host).
namespace {

static_assert(SPHX_FIELD_VEL_GRAD == 1u && SPHX_FIELD_DIVERGENCE == 2u && SPHX_FIELD_VORTICITY == 4u && SPHX_FIELD_COLOR_GRAD == 8u, "the field bits of the tile seam");
constexpr uint32_t FIELD_BITS_ALL = SPHX_FIELD_VEL_GRAD | SPHX_FIELD_DIVERGENCE | SPHX_FIELD_VORTICITY | SPHX_FIELD_COLOR_GRAD;

struct TileFieldsLayout {
    size_t at_wg, at_ids, at_g, at_d, at_w, at_c, words;
};
TileFieldsLayout tile_fields_layout(uint32_t n, uint32_t mask, bool ids) {
    const size_t nb = nblocks(n);
    TileFieldsLayout L;
    L.at_wg = 4 * nb;
    L.at_ids = L.at_wg + ((nb + 1 + 3) & ~(size_t)3);
    L.at_g = L.at_ids + (ids ? ((size_t)n + 1u) & ~(size_t)1u : 0u);
    L.at_d = L.at_g + (mask & SPHX_FIELD_VEL_GRAD ? 4 * (size_t)n : 0u);
    L.at_w = L.at_d + (mask & SPHX_FIELD_DIVERGENCE ? (size_t)n : 0u);
    L.at_c = L.at_w + (mask & SPHX_FIELD_VORTICITY ? (size_t)n : 0u);
    L.words = L.at_c + (mask & SPHX_FIELD_COLOR_GRAD ? 2 * (size_t)n : 0u);
    return L;
}
int tile_fields_scratch(sphx_ctx* c, size_t words) {
    if (words <= c->fields_cap && c->fields_buf) return SPHX_OK;
    SPHX_HIP(c, hipStreamSynchronize(c->stream));  // (a queued pass may still write the old buffer)
    c->fields_cap = 0;
    int rc;
    if ((rc = dev_alloc(c, &c->fields_buf, words))) return rc;
    c->fields_cap = words;
    return SPHX_OK;
}
// count + scan of the owned particles behind what is on the stream (pieces in array order: blockIdx.x)
void enqueue_fields_count(sphx_ctx* c, uint32_t n, uint32_t* wave_cnt, uint32_t* wg) {
    const uint32_t nb = nblocks(n);
    hipStream_t st = c->stream;
    launch(c, "tile_fields_count", 4.0 * n + 5.0 * 4.0 * nb, [&] { hipLaunchKernelGGL(sphx::k_fields_count, dim3(nb), dim3(256), 0, st, (const uint32_t*)c->pid, n, wave_cnt, wg); });
    launch(c, "tile_fields_scan", 8.0 * nb + 4.0, [&] { hipLaunchKernelGGL(sphx::k_remove_scan, dim3(1), dim3(256), 0, st, wg, nb); });
}
int tile_fields_check(sphx_ctx* c, const char* fn) {
    if (!c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "not a tile context (sphx_particle_fields serves a plain one)");
    return tile_sample_state(c, fn);
}

}  // namespace

extern "C" {

int sphx_tile_owned_count(sphx_ctx* c, uint32_t* out_owned) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_owned_count";
    if (!out_owned) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out_owned is NULL");
    *out_owned = 0;
    int rc;
    if ((rc = tile_fields_check(c, fn))) return rc;
    c->tfields.queued = false;  // (the scratch is shared with a queued query)
    const uint32_t n = c->N;
    if (!n) return SPHX_OK;
    SPHX_HIP(c, hipSetDevice(c->device));
    const TileFieldsLayout L = tile_fields_layout(n, 0u, false);
    if ((rc = tile_fields_scratch(c, L.words))) return rc;
    uint32_t* const buf = (uint32_t*)c->fields_buf;
    const uint32_t rev = c->K.rev;  // (launch() toggles the sweep direction of the step's next kernels: put back below)
    enqueue_fields_count(c, n, buf, buf + L.at_wg);
    c->K.rev = rev;
    uint32_t owned = 0;
    SPHX_HIP(c, hipMemcpyAsync(&owned, buf + L.at_wg + nblocks(n), 4, hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    if (owned > n) return c->fail(SPHX_ERR_HIP, fn, "the owned count is larger than the local count");
    *out_owned = owned;
    return SPHX_OK;
}

int sphx_tile_particle_fields_enqueue(sphx_ctx* c, uint32_t field_mask, uint32_t want_ids) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_particle_fields_enqueue";
    if (!field_mask) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "field_mask requests no output");
    if (field_mask & ~FIELD_BITS_ALL) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "unknown field_mask bits");
    int rc;
    if ((rc = tile_fields_check(c, fn))) return rc;
    c->tfields.queued = false;
    const uint32_t n = c->N;
    if (n) {
        SPHX_HIP(c, hipSetDevice(c->device));
        const TileFieldsLayout L = tile_fields_layout(n, field_mask, want_ids != 0u);
        if ((rc = tile_fields_scratch(c, L.words))) return rc;
        uint32_t* const buf = (uint32_t*)c->fields_buf;
        float* const fb = c->fields_buf;
        const FieldsArgs a{field_mask & SPHX_FIELD_VEL_GRAD ? fb + L.at_g : nullptr, field_mask & SPHX_FIELD_DIVERGENCE ? fb + L.at_d : nullptr,
                           field_mask & SPHX_FIELD_VORTICITY ? fb + L.at_w : nullptr, field_mask & SPHX_FIELD_COLOR_GRAD ? fb + L.at_c : nullptr};
        const sphx::FieldsOwned w{(const uint32_t*)c->pid, buf, buf + L.at_wg, want_ids ? buf + L.at_ids : nullptr};
        const bool vel = a.vel_grad || a.divergence || a.vorticity, col = a.color_grad != nullptr;
        const double bytes = (8.0 + (vel ? 8 : 0) + 4 + 4 + list_bytes(c) + (a.vel_grad ? 16 : 0) + (a.divergence ? 4 : 0) + (a.vorticity ? 4 : 0) + (col ? 8 : 0) + (want_ids ? 4 : 0)) * n;
        const uint32_t rev = c->K.rev;  // (launch() toggles the sweep direction of the step's next kernels: put back below)
        enqueue_fields_count(c, n, buf, buf + L.at_wg);
        hipStream_t st = c->stream;
        const dim3 g(nblocks(n)), b(256);
        launch(c, "tile_particle_fields", bytes, [&] {
            if (vel && col)
                hipLaunchKernelGGL((k_particle_fields_owned<true, true>), g, b, 0, st, c->pv(), (const float*)c->density, n, c->soff(), c->K, c->nbv(), a, w);
            else if (vel)
                hipLaunchKernelGGL((k_particle_fields_owned<true, false>), g, b, 0, st, c->pv(), (const float*)c->density, n, c->soff(), c->K, c->nbv(), a, w);
            else
                hipLaunchKernelGGL((k_particle_fields_owned<false, true>), g, b, 0, st, c->pv(), (const float*)c->density, n, c->soff(), c->K, c->nbv(), a, w);
        });
        c->K.rev = rev;
    }
    c->tfields.queued = true;
    c->tfields.n = n;
    c->tfields.mask = field_mask;
    c->tfields.ids = want_ids != 0u;
    return SPHX_OK;
}

int sphx_tile_particle_fields_fetch(sphx_ctx* c, const sphx_fields_out* out, uint32_t* ids, uint32_t cap, uint32_t* out_n) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_tile_particle_fields_fetch";
    if (!out || !out_n) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out or out_n is NULL");
    *out_n = 0;
    int rc;
    if ((rc = tile_fields_check(c, fn))) return rc;
    if (!c->tfields.queued) return c->fail(SPHX_ERR_NOT_READY, fn, "no sphx_tile_particle_fields_enqueue before it");
    const uint32_t mask = (out->vel_grad ? (uint32_t)SPHX_FIELD_VEL_GRAD : 0u) | (out->divergence ? (uint32_t)SPHX_FIELD_DIVERGENCE : 0u) |
                          (out->vorticity ? (uint32_t)SPHX_FIELD_VORTICITY : 0u) | (out->color_grad ? (uint32_t)SPHX_FIELD_COLOR_GRAD : 0u);
    if (mask != c->tfields.mask) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "out does not name the fields of the queued query");
    if (ids && !c->tfields.ids) return c->fail(SPHX_ERR_INVALID_ARGUMENT, fn, "ids asked for, but the queued query writes none");
    const uint32_t n = c->tfields.n;
    if (n != c->N) return c->fail(SPHX_ERR_NOT_READY, fn, "the particle set has changed since the enqueue");
    c->tfields.queued = false;
    if (!n) return SPHX_OK;
    SPHX_HIP(c, hipSetDevice(c->device));
    const TileFieldsLayout L = tile_fields_layout(n, mask, c->tfields.ids);
    const uint32_t* const buf = (const uint32_t*)c->fields_buf;
    hipStream_t st = c->stream;
    uint32_t k = 0;
    SPHX_HIP(c, hipMemcpyAsync(&k, buf + L.at_wg + nblocks(n), 4, hipMemcpyDeviceToHost, st));
    SPHX_HIP(c, hipStreamSynchronize(st));
    if (k > n) return c->fail(SPHX_ERR_HIP, fn, "the owned count is larger than the local count");
    *out_n = k;
    if (k > cap) return c->fail(SPHX_ERR_CAPACITY, fn, "the tile owns more particles than cap");
    if (!k) return SPHX_OK;
    if (ids) SPHX_HIP(c, hipMemcpyAsync(ids, buf + L.at_ids, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    if (out->vel_grad) SPHX_HIP(c, hipMemcpyAsync(out->vel_grad, buf + L.at_g, (size_t)k * 16, hipMemcpyDeviceToHost, st));
    if (out->divergence) SPHX_HIP(c, hipMemcpyAsync(out->divergence, buf + L.at_d, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    if (out->vorticity) SPHX_HIP(c, hipMemcpyAsync(out->vorticity, buf + L.at_w, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    if (out->color_grad) SPHX_HIP(c, hipMemcpyAsync(out->color_grad, buf + L.at_c, (size_t)k * 8, hipMemcpyDeviceToHost, st));
    SPHX_HIP(c, hipStreamSynchronize(st));
    return SPHX_OK;
}

}  // extern "C"
