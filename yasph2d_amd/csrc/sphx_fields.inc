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
template <bool VEL, bool COL>
__global__ NONP_BOUNDS void k_particle_fields(PVr PV, const float* __restrict__ density, uint32_t n, uint32_t soff, Consts K, NbView nb, FieldsArgs o) {
    __shared__ Stage<VEL ? 2 : 1, 1> rec;  // position (, velocity); volume
    const uint32_t blk = xcd_bid(K.rev, K.xcd_shift);
    const uint32_t i = blk * 256 + threadIdx.x;
    NbHead h = nb_head(nb, blk, i, n);
    struct Rec {
        float4 pv;  // (z, w unused without VEL)
        float vol;
    };
    const float vol_b = K.mass / K.rho0;
    auto pv_of = [&](uint32_t g) {
        if constexpr (VEL) {
            return ldpv(PV, g);
        } else {
            const float2 p = gat(PV.pos, g);
            return make_float4(p.x, p.y, 0.0f, 0.0f);
        }
    };
    auto load = [&](uint32_t g) {
        const float rho = gat(density, g < soff ? g : 0u);  // (clamped, not predicated: no branch between the loads)
        return Rec{pv_of(g), g < soff ? K.mass / rho : vol_b};
    };
    auto load2 = [&](uint32_t g) {
        Pair<float4> pv;
        if constexpr (VEL) {
            pv = ldpv2(PV, g);
        } else {
            const Pair<float2> p = gat2(PV.pos, g);
            pv = Pair<float4>{make_float4(p.a.x, p.a.y, 0.0f, 0.0f), make_float4(p.b.x, p.b.y, 0.0f, 0.0f)};
        }
        const Pair<float> rho = gat2(density, g < soff ? g : 0u);  // (a pair that straddles soff: the second record is a boundary particle's)
        return Pair<Rec>{Rec{pv.a, g < soff ? K.mass / rho.a : vol_b}, Rec{pv.b, g + 1u < soff ? K.mass / rho.b : vol_b}};
    };
    nb_stage(h, nb, blk, i, n, load, load2, [&](uint32_t slot, const Rec& r) {
        if constexpr (VEL)
            rec.put_vec01(slot, r.pv);
        else
            rec.template put_vec<0>(slot, make_float2(r.pv.x, r.pv.y));
        rec.template put_scal<0>(slot, r.vol);
    });
    __syncthreads();
    if (i >= n) return;
    auto take = [&](uint32_t off) {
        if constexpr (VEL) {
            return Rec{rec.vec01(off), rec.template scal<0>(off)};
        } else {
            const float2 p = rec.template vec<0>(off);
            return Rec{make_float4(p.x, p.y, 0.0f, 0.0f), rec.template scal<0>(off)};
        }
    };
    const float4 pvi = h.wide ? pv_of(i) : take((i - h.lw0) * 4u).pv;
    const float2 ri = make_float2(pvi.x, pvi.y);
    float lxx = 0.0f, lxy = 0.0f, lyx = 0.0f, lyy = 0.0f, cx = 0.0f, cy = 0.0f;
    auto walk = [&](auto fast) {
        auto consume = [&](const Rec& r, uint32_t) {
            const float2 g = wendland_grad<decltype(fast)::value>(K, ri, make_float2(r.pv.x, r.pv.y));
            const float ax = r.vol * g.x, ay = r.vol * g.y;
            if (VEL) {
                const float dvx = r.pv.z - pvi.z, dvy = r.pv.w - pvi.w;
                lxx = lxx + dvx * ax;
                lxy = lxy + dvx * ay;
                lyx = lyx + dvy * ax;
                lyy = lyy + dvy * ay;
            }
            if (COL) {
                cx = cx + ax;
                cy = cy + ay;
            }
        };
        nb_traverse(h, h.ct, take, load, consume);
    };
    if (K.q_noclamp)  // (kernel argument: a scalar branch; sqrt_dist — both forms are correctly rounded, so both give the contract's bits)
        walk(std::true_type{});
    else
        walk(std::false_type{});
    if (VEL) {
        if (o.vel_grad) {  // (the outputs may be the caller's device arrays: only 4-byte alignment is assumed)
            float* p = o.vel_grad + 4 * (size_t)i;
            p[0] = lxx;
            p[1] = lxy;
            p[2] = lyx;
            p[3] = lyy;
        }
        if (o.divergence) o.divergence[i] = lxx + lyy;
        if (o.vorticity) o.vorticity[i] = lyx - lxy;
    }
    if (COL && o.color_grad) {
        o.color_grad[2 * (size_t)i] = cx;
        o.color_grad[2 * (size_t)i + 1] = cy;
    }
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
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_particle_fields: not available on a tile context (its arrays hold ghosts and miss the particles other tiles own)");
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
