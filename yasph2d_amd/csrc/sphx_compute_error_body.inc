// The body of k_compute_error and of k_compute_error_rigid (sphx_kernels.hip has the story of both), included where DIVERGENCE,
// PREDICT, KNZ, TAKE and RIGID are compile-time constants and the kernel arguments are in scope.  A textual body and not a function:
// the staging area is a __shared__ object of the kernel, and an instantiation with RIGID = 0 keeps the code it had as a kernel body.
// RIGID (k_compute_error_rigid only; 1: accel[] from the arguments, 2: and the fluid-only exit) is described in front of that kernel.
    static_assert(!TAKE || KNZ, "the take-over producers are the ones that leave flags");
    constexpr bool SPEC = TAKE && !DIVERGENCE;  // (the speculative cell count)
    // device-run loop: an iteration queued behind the one that met the residual test has nothing to do
    if (la.enabled && la.iter > 1u && scal->loop_done != 0u) return;
    if (dt_dev) dt = *dt_dev;
    // Every density correction of a device-run loop also does the re-grid's cell count (it cannot know early and cheaply whether it
    // is the last one: deriving the verdict in every workgroup cost that kernel 2.5 us).  This iteration exists, so the previous
    // correction was not the last: its count is wiped here, a slice per workgroup, before this iteration's correction counts again.
    if (clear_hist) {
        const uint32_t per = (clear_len + gridDim.x - 1u) / gridDim.x;
        const uint32_t c0 = blockIdx.x * per, c1 = min(c0 + per, clear_len);
        for (uint32_t k = c0 + threadIdx.x; k < c1; k += 256u) clear_hist[k] = 0u;
    }
    __shared__ Stage<2, 0> rec;  // position, velocity
    auto put = [&](uint32_t slot, const float4& r) { rec.put_vec01(slot, r); };
    auto take = [&](uint32_t o) { return rec.vec01(o); };
    const uint32_t blk = xcd_bid(K.rev, K.xcd_shift);
    const uint32_t i = blk * 256 + threadIdx.x;
    [[maybe_unused]] bool k_a = false;  // RIGID: accel[] was not written and stands for K.a (the verdict word carries this launch's tag)
    if constexpr (RIGID != 0) {
        static_assert(!DIVERGENCE && PREDICT && KNZ && TAKE, "the rigid form is the density loop's take-over producer with the prediction");
        // ---- first batch: nothing in it depends on anything else.  (clamped, not predicated: nb_head)
        uint32_t vb = 0;
        if (pa.va.enabled && threadIdx.x < STRIPES) vb = scal->vstripe[threadIdx.x].vmax[pa.va.vslot & 3u];
        const uint32_t verdict = scal->verdict.accel_uniform;  // (plain loads of wave-uniform addresses: the pass in front has finished)
        const float2 v0 = PV.vel[0];
        const uint32_t last = n ? n - 1u : 0u, ic = min(i, last);
        const uint32_t craw = nb.counts[ic];
        const uint32_t wi = (uint32_t)__builtin_amdgcn_readfirstlane(i >> 6);
        const uint32_t ww = wi * 64u < n ? nb.wave[wi] : 0u;
        const float2 p_i = PV.pos[ic];
        const float rho_r = density[ic], alpha_r = alpha[ic];
        // ---- the timer law, as the walk's form below runs it
        __shared__ float dt_r;
        if (pa.va.enabled && threadIdx.x < 64) {
            const uint32_t b = wave_max_u32(vb);
            const unsigned long long ns = timer_law_step_ns(pa.law, sqrtf(__uint_as_float(b)));
            const float d = duration_as_secs_f32(ns);
            if (threadIdx.x == 0) dt_r = d;
            if (blockIdx.x == 0) vmax_publish(scal, pa.va, b, pa.law, ns, d);
        }
        if (pa.va.enabled) {
            __syncthreads();
            dt = dt_r;
        }
        k_a = verdict == ta.accel_tag;
        // v* of every fluid particle: predicted()'s two operations on vel[0] and K.a
        const float4 pvi = make_float4(p_i.x, p_i.y, v0.x + K.ax * dt, v0.y + K.ay * dt);
        const bool finite = ((__float_as_uint(pvi.z) & 0x7f800000u) != 0x7f800000u) && ((__float_as_uint(pvi.w) & 0x7f800000u) != 0x7f800000u);
        DirAhead ahead_r{0xFFFFFFFFu, EMPTY};
        if constexpr (RIGID == 2) {
            if (ta.hist && i < n) {  // the directory entry in front of the count: in flight across the barrier below
                uint32_t cx0, cy0;
                cell_of(K, p_i, cx0, cy0);
                ahead_r = dir_ahead(ta.g, cx0, cy0);
            }
        }
        const uint32_t c = i < n ? craw : 0u;
        const bool reaches_static = (c & 0x7fu) != ((c >> 7) & 0x7fu) || (ww >> 31) != 0u;  // ct != cd, or a wide wavefront
        const bool walks = __syncthreads_or(reaches_static ? 1 : 0) != 0 || !k_a || !finite || RIGID != 2;
        if (ta.count && threadIdx.x == 0) {  // (the grid is rounded up: only workgroups that hold a particle are counted)
            Stripe& s = scal->stripe[blockIdx.x % STRIPES];
            if (k_a && blk * 256u < n) atomicAdd(walks ? &s.rp_walk : &s.rp_exit, 1u);
            if (!k_a && blockIdx.x == 0) atomicAdd(&s.rp_noverdict, 1u);
        }
        if (!walks) {
            // The walk's tail below, statement for statement, on the same values (a copy and not a shared lambda: with one, the
            // instantiations without RIGID lost the instruction streams they had).
            float e = 0.0f, e_owned = 0.0f;
            uint32_t k_bits = 0u;
            float2 pnew = make_float2(0.0f, 0.0f);
            if (i < n) {
                const float delta = 0.0f;  // the walk's sum: +0 + (+-0) ... = +0
                e = rho_r + delta * K.mass * dt;  // dfsph.rs:121
                e = fmaxf(K.rho0, e) - K.rho0;    // dfsph.rs:124
                const float kv = e * alpha_r;
                kbuf[i] = kv;
                k_bits = __float_as_uint(kv);
                pa.vel_out[i] = make_float2(pvi.z, pvi.w);
                store_cold(&warm_zero[i], 0.0f + kv, K.nt_cold);
                e_owned = tile_owns(K, pvi.x, pvi.y) ? e : 0.0f;
                pnew = make_float2(pvi.x + pvi.z * dt, pvi.y + pvi.w * dt);
            }
            if (ta.hist) count_cell(K, ta.g, i < n, i, pnew, ta.hist, ta.cidx, 1u, scal, ahead_r, &scal->spec.flags);
            knz_store(knz, i, k_bits, scal, knz_tag);
            block_residual_add(e_owned, scal);
            return;
        }
    }
    NbHead h = nb_head(nb, blk, i, n);
    // this particle's scalars are requested together with everything else (one round trip, not two)
    const float rho_i = (!DIVERGENCE && i < n) ? density[i] : 0.0f;
    const float alpha_i = i < n ? alpha[i] : 0.0f;
    struct PredRec {
        float4 pv;
        float2 a;
    };
    auto load_pred = [&](uint32_t g) {
        if constexpr (RIGID != 0) {  // (a wave-uniform branch: no accel word is requested under the verdict)
            if (k_a) return PredRec{ldpv(PV, g), make_float2(K.ax, K.ay)};
        }
        return PredRec{ldpv(PV, g), gat(pa.accel, g < soff ? g : 0u)};  // accel[] has no boundary tail
    };
    auto predicted = [&](const PredRec& r, uint32_t g) {  // dfsph.rs:484-492, the operations of k_predict; boundary records keep v = 0
        return g < soff ? make_float4(r.pv.x, r.pv.y, r.pv.z + r.a.x * dt, r.pv.w + r.a.y * dt) : r.pv;
    };
    if (PREDICT) {
        // The reduction's stripes are requested FIRST (loads return in order: behind the staging loads the maximum would arrive last),
        // then all records; the first wavefront applies the timer law while the records are in flight.
        // (pa.va.enabled == 0 — tile path: dt is the host's, all-reduced over the tiles; no law here)
        // (RIGID: the law has run in front of the decision)
        uint32_t vb = 0;
        if (RIGID == 0 && pa.va.enabled && threadIdx.x < STRIPES) vb = scal->vstripe[threadIdx.x].vmax[pa.va.vslot & 3u];
        // (a pair that straddles soff: its second record is a boundary particle's, predicted() ignores the acceleration it got)
        auto load_pred2 = [&](uint32_t g) {
            const Pair<float4> pv = ldpv2(PV, g);
            if constexpr (RIGID != 0) {
                if (k_a) return Pair<PredRec>{PredRec{pv.a, make_float2(K.ax, K.ay)}, PredRec{pv.b, make_float2(K.ax, K.ay)}};
            }
            const Pair<float2> a = gat2(pa.accel, g < soff ? g : 0u);
            return Pair<PredRec>{PredRec{pv.a, a.a}, PredRec{pv.b, a.b}};
        };
        const NbStaged<PredRec> st = nb_stage_load(h, nb, blk, i, n, load_pred, load_pred2);
        __shared__ float dt_s;
        if (RIGID == 0 && pa.va.enabled && threadIdx.x < 64) {
            const uint32_t b = wave_max_u32(vb);
            const unsigned long long ns = timer_law_step_ns(pa.law, sqrtf(__uint_as_float(b)));
            const float d = duration_as_secs_f32(ns);
            if (threadIdx.x == 0) dt_s = d;
            if (blockIdx.x == 0) vmax_publish(scal, pa.va, b, pa.law, ns, d);
        }
        if (RIGID == 0 && pa.va.enabled) {
            __syncthreads();
            dt = dt_s;
        }
        nb_stage_store(h, st, [&](uint32_t slot, const PredRec& r, uint32_t g) { put(slot, predicted(r, g)); });
    } else {
        nb_stage(h, nb, blk, i, n, [&](uint32_t g) { return ldpv(PV, g); }, [&](uint32_t g) { return ldpv2(PV, g); }, put);
    }
    __syncthreads();
    float e = 0.0f, e_owned = 0.0f;
    uint32_t k_bits = 0u;
    [[maybe_unused]] float2 pnew = make_float2(0.0f, 0.0f);
    [[maybe_unused]] DirAhead ahead{0xFFFFFFFFu, EMPTY};
    if (i < n) {
        const uint32_t ct = h.ct;
        float4 pvi = h.wide ? ldpv(PV, i) : take((i - h.lw0) * 4u);
        if (PREDICT && h.wide) pvi = predicted(load_pred(i), i);
        if constexpr (SPEC) {
            if (ta.hist) {  // the directory entry of the block the particle is in now, requested in front of the walk (k_correct)
                uint32_t cx0, cy0;
                cell_of(K, make_float2(pvi.x, pvi.y), cx0, cy0);
                ahead = dir_ahead(ta.g, cx0, cy0);
            }
        }
        if (!(DIVERGENCE && ct < 9)) {  // dfsph.rs:261
            const float2 ri = make_float2(pvi.x, pvi.y);
            float delta = 0.0f;
            auto walk = [&](auto fast) {
                auto consume = [&](const float4& r, uint32_t) {
                    const float2 g = wendland_grad<decltype(fast)::value>(K, ri, make_float2(r.x, r.y));
                    // boundary records carry v = 0, so v_i - 0 = v_i is the static form of dfsph.rs:118 / :274
                    const float dvx = pvi.z - r.z, dvy = pvi.w - r.w;
                    delta = delta + (dvx * g.x + dvy * g.y);
                };
                nb_traverse(h, ct, take, [&](uint32_t g) { return PREDICT ? predicted(load_pred(g), g) : ldpv(PV, g); }, consume);
            };
            if (K.q_noclamp)  // (kernel argument: a scalar branch; sqrt_dist)
                walk(std::true_type{});
            else
                walk(std::false_type{});
            if (DIVERGENCE) {
                e = fmaxf(delta * K.mass, 0.0f);  // dfsph.rs:277-278
            } else {
                e = rho_i + delta * K.mass * dt;  // dfsph.rs:121
                e = fmaxf(K.rho0, e) - K.rho0;         // dfsph.rs:124
            }
        }
        const float kv = e * alpha_i;
        kbuf[i] = kv;  // k = err * alpha: all the correction needs of a neighbour besides its position
        k_bits = __float_as_uint(kv);
        // the predicted velocity of the own particle (staged with the window).  Stored HERE, behind the walk: a store in front of it
        // sits in the same counter as the walk's entry loads, and every wait for one of those waited for the store's acknowledge too
        if (PREDICT) pa.vel_out[i] = make_float2(pvi.z, pvi.w);
        if constexpr (TAKE)
            store_cold(&warm_zero[i], 0.0f + kv, K.nt_cold);  // dfsph.rs:296 behind :361-363
        else if (warm_zero)
            warm_zero[i] = 0.0f;  // dfsph.rs:206-208 / 361-363 (callers whose first correction does not start from zero itself)
        e_owned = tile_owns(K, pvi.x, pvi.y) ? e : 0.0f;
        if constexpr (SPEC) pnew = make_float2(pvi.x + pvi.z * dt, pvi.y + pvi.w * dt);  // dfsph.rs:499-510, as the quiet exit of k_correct
    }
    if constexpr (SPEC)
        if (ta.hist) count_cell(K, ta.g, i < n, i, pnew, ta.hist, ta.cidx, 1u, scal, ahead, &scal->spec.flags);
    if constexpr (KNZ) knz_store(knz, i, k_bits, scal, knz_tag);  // (the grid is rounded up to whole workgroups, and so is knz[])
    block_residual_add(e_owned, scal);  // read by the correction queued behind this launch (ResArgs)
