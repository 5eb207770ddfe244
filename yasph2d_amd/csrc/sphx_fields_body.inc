// sphx_fields_body.inc — the body of k_particle_fields<VEL, COL> and k_particle_fields_owned<VEL, COL> (sphx_fields.inc), included once
// into each with SPHX_FIELDS_OWNED 0 / 1: the plain form is the text it always was and compiles to the instructions it always did
// (profiles/fields_multi/isa.txt).  In scope: PV, density, n, soff, K, nb, o (FieldsArgs) and, in the owned form, w (FieldsOwned).
    __shared__ Stage<VEL ? 2 : 1, 1> rec;  // position (, velocity); volume
    const uint32_t blk = xcd_bid(K.rev, K.xcd_shift);
    const uint32_t i = blk * 256 + threadIdx.x;
#if SPHX_FIELDS_OWNED
    // a piece without an owned particle: nothing to answer (blk is the same for the whole workgroup: a scalar test, and nobody waits at
    // the barrier below)
    const uint32_t piece_off = w.wg_off[blk];
    if (w.wg_off[blk + 1u] == piece_off) return;
#endif
    NbHead h = nb_head(nb, blk, i, n);
#if SPHX_FIELDS_OWNED
    const uint32_t raw = w.pid[min(i, n - 1u)];  // (clamped like the head's loads; n > 0: an empty tile launches nothing)
    const bool own = i < n && (raw >> 31) != 0u;
    uint32_t dst;  // the particle's place among the owned ones of the tile
    {
        const unsigned long long m = __ballot(own);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const uint4 cnt = *(const uint4*)(w.wave_cnt + 4u * (size_t)blk);  // (16-byte aligned: the scratch's first words)
        dst = piece_off + (wv > 0u ? cnt.x : 0u) + (wv > 1u ? cnt.y : 0u) + (wv > 2u ? cnt.z : 0u) + rank;
        if (own && w.ids) w.ids[dst] = raw & 0x7FFFFFFFu;
    }
#endif
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
#if SPHX_FIELDS_OWNED
        nb_traverse(h, own ? h.ct : 0u, take, load, consume);  // (a ghost walks nothing: nb_traverse masks by lim)
#else
        nb_traverse(h, h.ct, take, load, consume);
#endif
    };
    if (K.q_noclamp)  // (kernel argument: a scalar branch; sqrt_dist — both forms are correctly rounded, so both give the contract's bits)
        walk(std::true_type{});
    else
        walk(std::false_type{});
#if SPHX_FIELDS_OWNED
    if (!own) return;  // a ghost is never written
    const uint32_t at = dst;
#else
    const uint32_t at = i;
#endif
    if (VEL) {
        if (o.vel_grad) {  // (the outputs may be the caller's device arrays: only 4-byte alignment is assumed)
            float* p = o.vel_grad + 4 * (size_t)at;
            p[0] = lxx;
            p[1] = lxy;
            p[2] = lyx;
            p[3] = lyy;
        }
        if (o.divergence) o.divergence[at] = lxx + lyy;
        if (o.vorticity) o.vorticity[at] = lyx - lxy;
    }
    if (COL && o.color_grad) {
        o.color_grad[2 * (size_t)at] = cx;
        o.color_grad[2 * (size_t)at + 1] = cy;
    }
