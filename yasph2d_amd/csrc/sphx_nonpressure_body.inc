// The body of the non-pressure pass for one block of 256 particles (dfsph.rs:436-477): included by k_nonpressure, which runs it once
// for the block its workgroup number maps to, and by k_nonpressure_rigid, which runs it in a loop over the virtual blocks of its
// workgroup when a mark says the fluid is not in rigid motion (sphx_kernels.hip has the story of both).  A textual body and not a
// function, for the reason sphx_correct_body.inc is one: k_nonpressure keeps its instruction stream.
// The includer provides, besides the kernel's parameters and VM: rec (the staging area, __shared__ Stage<2, 1>) and blk (the block).
// It leaves vsq = |v_i + a_i dt|^2 of the lane's particle (0 for a lane without one) for the includer's reduction.
    const uint32_t i = blk * 256 + threadIdx.x;
    NbHead h = nb_head(nb, blk, i, n);
    struct StageRec {
        float4 pv;
        float rho;
    };
    nb_stage(
        h, nb, blk, i, n, [&](uint32_t g) { return StageRec{ldpv(PV, g), gat(density, g < soff ? g : 0u)}; },  // density[] has no boundary tail (XSPH: dynamic neighbours only, dfsph.rs:456)
        [&](uint32_t g) {
            const Pair<float4> pv = ldpv2(PV, g);
            const Pair<float> rho = gat2(density, g < soff ? g : 0u);  // (a pair that straddles soff: the second record is a boundary particle's, its density is not used)
            return Pair<StageRec>{StageRec{pv.a, rho.a}, StageRec{pv.b, rho.b}};
        },
        [&](uint32_t slot, const StageRec& r) {
            rec.put_vec01(slot, r.pv);
            rec.put_scal<0>(slot, r.rho);
        });
    __syncthreads();
    float vsq = 0.0f;
    if (i < n) {
        const uint32_t oi = (i - h.lw0) * 4u;
        const float4 pvi = h.wide ? ldpv(PV, i) : rec.vec01(oi);
        const uint32_t cd = h.cd;
        float ax = K.ax, ay = K.ay;
        struct Rec {
            float4 pv;
            float rho;
        };
        if constexpr (VM == SPHX_VISCOSITY_PHYSICAL) {
            // the same walk with r = sqrt(r_sq) (dfsph.rs:461): only ALU is added, the staged record already holds everything
            const float mu_m = V.mu * K.mass;
            auto walk = [&](auto fast) {
                auto consume = [&](const Rec& r, uint32_t) {
                    const float dx = r.pv.x - pvi.x, dy = r.pv.y - pvi.y;
                    const float r_sq = dx * dx + dy * dy;
                    const float f = physical_visc(K, V, mu_m, sqrt_dist<decltype(fast)::value>(r_sq), r.rho);
                    ax = ax + f * (r.pv.z - pvi.z);
                    ay = ay + f * (r.pv.w - pvi.w);
                };
                nb_traverse(
                    h, cd, [&](uint32_t o) { return Rec{rec.vec01(o), rec.scal<0>(o)}; },
                    [&](uint32_t g) { return Rec{ldpv(PV, g), gat(density, g)}; }, consume);
            };
            if (K.q_noclamp)  // (kernel argument: a scalar branch; sqrt_dist)
                walk(std::true_type{});
            else
                walk(std::false_type{});
        } else {
            const float em = K.xsph_eps * K.mass;
            auto consume = [&](const Rec& r, uint32_t) {
                const float dx = r.pv.x - pvi.x, dy = r.pv.y - pvi.y;
                const float r_sq = dx * dx + dy * dy;
                const float f = em * poly6_eval(K, r_sq) / (r.rho * dt);
                ax = ax + f * (r.pv.z - pvi.z);
                ay = ay + f * (r.pv.w - pvi.w);
            };
            nb_traverse(
                h, cd, [&](uint32_t o) { return Rec{rec.vec01(o), rec.scal<0>(o)}; },
                [&](uint32_t g) { return Rec{ldpv(PV, g), gat(density, g)}; }, consume);
        }
        accel[i] = make_float2(ax, ay);
        const float px = pvi.z + ax * dt, py = pvi.w + ay * dt;
        vsq = tile_owns(K, pvi.x, pvi.y) ? px * px + py * py : 0.0f;  // ghosts of a tile are somebody else's particles
    }
