// The body of a velocity correction for one block of 256 particles: included by k_correct, which runs it once for the block its
// workgroup number maps to, and by k_correct_thin, which runs it in a loop over the virtual blocks of its workgroup (sphx_kernels.hip
// has the story of both).  A textual body and not a function: behind a function boundary the compiler schedules the instantiations
// of k_correct differently (up to 6 VGPRs more), and those are tuned kernels.
// The includer provides, besides the kernel's parameters and WARM / INV_DT / TILE / ZS / QF:
//   THIN  (constexpr bool) and, used with THIN only, vblk (the virtual block), vgrid (their number) and look (the workgroup's first
//         block: the one in front of which it reads the marks; vblk == 0 is the judge);
//   SPHX_CORRECT_LEAVE(quiet): leaves the body — quiet: through the quiet exit.
    static_assert(!ZS || (!WARM && !TILE), "the skip belongs to the plain corrections");
    static_assert(!QF || ZS, "the decide-first form falls back to the skip's decision");
    float dt = WARM ? ca.dt : (la.enabled ? la.dt : ca.dt);
    if (dt_dev) {
        dt = *dt_dev;
        inv_dt = 1.0f / dt;
    }
    // This launch sits right behind its iteration's compute_error and READS the residual sum that one left in the stripes (ResArgs):
    // the first wavefront of workgroup 0 keeps the books (snapshot of the cumulative sums), applies the test of dfsph.rs:221-236 /
    // :376-391 in a device-run loop (LoopArgs; DevScalars::loop_done) and publishes to the mailbox.  The stripes are requested
    // first and reduced late, so they cost no round trip of their own.
    constexpr bool RES = !WARM;
    const bool need_verdict = RES && ra.enabled && (THIN ? vblk == 0u : blockIdx.x == 0);
    const bool judge = need_verdict && threadIdx.x < 64;
    unsigned long long hi = 0, lo = 0, snap_h = 0, snap_l = 0;
    uint32_t sticky = 0;
    uint32_t jmark = ~ra.rseq;  // ZS, the judging wavefront: the scene-wide mark of one stripe
    const uint32_t rp = ra.rseq & 1u;
    if (RES && ra.enabled) {
        // device-run loop: an iteration queued behind the one that met the residual test has nothing to do
        const uint32_t done_before = (la.enabled && la.iter > 1u) ? scal->loop_done : 0u;
        if (judge) {  // everything the verdict needs is requested here, in one round trip, ahead of the staging loads
            residual_stripe_load(scal, hi, lo);
            if constexpr (ZS)
                if (threadIdx.x < STRIPES) jmark = scal->mstripe[threadIdx.x].knz_mark;
            snap_h = scal->snap_hi[rp ^ 1u];
            snap_l = scal->snap_lo[rp ^ 1u];
            sticky = scal->flags;
        }
        if (done_before != 0u && done_before < la.iter) {  // (== iter: workgroup 0 of THIS launch has just recorded its verdict)
            if (blockIdx.x == 0 && threadIdx.x < 64) {  // nothing was added since: the snapshot chain stays intact
                residual_wave_reduce(hi, lo);
                if (threadIdx.x == 0) {
                    scal->snap_hi[rp] = hi;
                    scal->snap_lo[rp] = lo;
                }
            }
            SPHX_CORRECT_LEAVE(false);
        }
    }
    // staged per neighbour: its position and ONE scalar — WARM: its warm-start value; else k = err * alpha of this iteration
    // (12 bytes a record; round 1 kept a packed {pos, k, err} float4 for one-gather-per-neighbour access, which the LDS staging made
    // pointless: 16 bytes written per particle by compute_error, 16 staged per record here)
    __shared__ Stage<1, 1> rec;  // position; the scalar
    const float* const wsrc = WARM ? (const float*)warm : kbuf;
    struct StageRec {
        float2 p;
        float w;
    };
    // warm[] / kbuf[] have no boundary tail.  A boundary record is staged with the scalar 0: its term is k_i alone (dfsph.rs:156 /
    // :188 / :309 / :339), and k_i + 0 = k_i to the bit (WARM: 0.5 max(0, lim) = 0, lim < 0) — so the walk adds (k_i + k_j) for every
    // entry and needs no "dynamic or static?" select per neighbour (round 4: add + compare + select, 10 cycles of ~100).  (k_i = -0
    // would become +0: the sign of a zero summand never reaches the sum, which starts from +0 and therefore is never -0.)
    // (the zero is selected when the record is STORED: a select behind the load would make the compiler wait for the load right
    // there — inside the branch of nb_stage_load's second round of table lines)
    auto load_rec = [&](uint32_t g) { return StageRec{gat(posA, g), gat(wsrc, g < soff ? g : 0u)}; };
    auto load_rec2 = [&](uint32_t g) {
        const Pair<float2> p = gat2(posA, g);
        const Pair<float> w = gat2(wsrc, g < soff ? g : 0u);  // (a pair that straddles soff: store_rec zeroes the boundary record's scalar)
        return Pair<StageRec>{StageRec{p.a, w.a}, StageRec{p.b, w.b}};
    };
    auto store_rec = [&](uint32_t slot, const StageRec& q, uint32_t g) {
        rec.put_vec<0>(slot, q.p);
        rec.put_scal<0>(slot, g < soff ? q.w : 0.0f);
    };
    // Everything the block needs from global memory, requested in one go (Loaded).  (Round 5 tried workgroups that do TWO consecutive
    // blocks, the second block's requests going out before the first block's walk begins: 64 registers, eight workgroups per CU
    // kept — and slower at both sizes, 174.7 against 169.6 us at 16 M, 15.6 against 12.7 us at 1 M:
    // profiles/r05_experiments/two_blocks_per_workgroup.txt.)
    struct Loaded {
        uint32_t blk, i;
        NbHead h;
        float4 pvi;
        float warm_i;
        uint32_t id_i;
        NbStaged<StageRec> st;
        DirAhead ahead;
    };
    // (two parts: the head — list words, table lines, the own particle's words — and the staging loads.  Between them sits the
    // zero-correction skip's decision: its flag words are requested in front of the head and looked at behind it, so a workgroup that
    // walks has lost no round trip to them, and the table lines a clear window's second look needs are the head's)
    auto load_head = [&](uint32_t blk) {
        Loaded L;
        L.blk = blk;
        L.i = blk * 256 + threadIdx.x;
        L.h = nb_head(nb, blk, L.i, n);
        // (the own particle, round 6: only the velocity — the position is in the window this workgroup stages, process() takes it from there: one 8-byte
        // load per thread less, 16 cycles of the CU's address path per wavefront, tools/vmem_issue_bench.hip)
        {
            const float2 vi = gat((const float2*)vel, min(L.i, n ? n - 1u : 0u));
            L.pvi = make_float4(0.0f, 0.0f, vi.x, vi.y);
        }
        // first: the first correction of its loop — the accumulated warm-start value starts from zero (dfsph.rs:206-208 / :361-363):
        // nothing is read, and nobody had to write that zero either
        // (clamped, not predicated on i < n: behind that branch the compiler also selects the count word — and waits for it there)
        if constexpr (ZS)
            L.warm_i = first ? 0.0f : warm[min(L.i, n ? n - 1u : 0u)];
        else  // (the kernels without the skip's decision keep the predicated form they were tuned with)
            L.warm_i = (L.i < n && !first) ? warm[L.i] : 0.0f;
        // (TILE — TileClassArgs in use: clamped, not predicated; behind a branch the compiler tests the owner bit inside it and waits there)
        L.id_i = TILE ? tc.pid[min(L.i, n - 1u)] : 0u;
        return L;
    };
    auto load_stage = [&](Loaded& L) {
        L.st = nb_stage_load(L.h, nb, L.blk, L.i, n, load_rec, load_rec2);
        L.ahead = DirAhead{0xFFFFFFFFu, EMPTY};  // (requested in process(), once the position is there)
    };
    auto verdict = [&] {
    if (judge) {
        constexpr bool DIVERGENCE = !INV_DT;
        residual_wave_reduce(hi, lo);
        const double sum64 = residual_sum_f64(hi, lo, snap_h, snap_l);
        bool more = false;
        if (la.enabled) {
            // the host's operations: f64 sum rounded once, two f32 divisions, one product
            const float sum = (float)sum64;
            const float avg = DIVERGENCE ? sum / (float)la.n_total / la.rho0 : sum / (float)la.n_total;
            if ((sticky & DF_NONFINITE) || !(fabsf(avg) <= 3.402823466e38f)) {
                more = false;  // the reference panics (dfsph.rs:223 / :378); the host reports it
            } else if (la.fixed) {
                more = la.iter < la.fixed;
            } else {
                const float rel = DIVERGENCE ? avg : avg / la.rho0;  // dfsph.rs:222
                more = !(rel * dt < la.tol);                         // dfsph.rs:226 / :381
                if (more && la.iter > la.max_iters) more = false;    // dfsph.rs:236 / :391
            }
        }
        // ZS: what the host's hint for this loop's next corrections is made from (a launch without flags knows of no mark)
        [[maybe_unused]] const bool marked = ZS ? __any(jmark == ra.rseq) != 0 : true;
        if (blockIdx.x == 0) {
            if (threadIdx.x == 0) {
                scal->snap_hi[rp] = hi;
                scal->snap_lo[rp] = lo;
                ra.mb->err_sum = sum64;
                if constexpr (ZS) ra.mb->quiet_seq = (zs.knz && !marked) ? ra.seq : 0u;
                if (la.enabled) {
                    ra.mb->loop_hist[la.iter % LOOP_HIST] = sum64;
                    __hip_atomic_store(&scal->loop_done, more ? 0u : la.iter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (!more) {
                        ra.mb->loop_iters = la.iter;
                        __threadfence_system();
                        __hip_atomic_store((uint32_t*)&ra.mb->loop_gen_done, la.gen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                }
            }
            publish_common(scal, ra.mb, ra.seq);
        }
    }
    };
    const uint32_t blk0 = THIN ? xcd_map(vblk, vgrid, K.rev, K.xcd_shift) : xcd_bid(K.rev, K.xcd_shift);
    // quiet scene: the mark is requested in front of everything else and looked at before the head is issued.  The scalar conditions
    // are the skip's (zs.knz stands for K.q_noclamp, no tile, a positive finite mass: launch_correct).
    if constexpr (QF) {
        const uint32_t b0 = blk0 * 256u;
        // (THIN: a workgroup looks once, in front of its first block, and the answer holds for all of them — an empty block included)
        if (zs.knz && (THIN ? look : b0 < n) && (!INV_DT || (inv_dt > 0.0f && inv_dt <= 3.402823466e38f))) {
            __shared__ uint32_t quiet_s;
            // (one wavefront reads the stripes, as the velocity prediction reads its maximum: every workgroup sees the same 32 words,
            // nobody writes them while this launch runs, and the XCD's L2 serves them)
            uint32_t mk = ~ra.rseq;
            if (threadIdx.x < STRIPES) mk = scal->mstripe[threadIdx.x].knz_mark;
            const uint32_t i = b0 + threadIdx.x, ic = min(i, n - 1u);
            const float2 vi = INV_DT && !THIN ? gat((const float2*)vel, ic) : make_float2(0.0f, 0.0f);
            const float2 pi = INV_DT && !THIN ? gat(posA, ic) : make_float2(0.0f, 0.0f);
            // first: the sum starts from +0 and k_i is +0 or -0 — (+0) + (+0) = +0 and (+0) + (-0) = +0 in round-to-nearest, the bits
            // 0x00000000 either way, which is what `0.0f + k_i` of the skip's exit below stores.  Neither word is read.
            const float warm_i = (THIN || first) ? 0.0f : warm[ic];
            const float ki = (THIN || first) ? 0.0f : kbuf[ic];
            if (threadIdx.x < 64) {
                const bool marked = __any(mk == ra.rseq) != 0;
                if (threadIdx.x == 0) quiet_s = marked ? 0u : 1u;
            }
            __syncthreads();
            if constexpr (THIN && INV_DT) {  // marked: the speculative flags are dropped unmerged, the recount raises the real ones
                if (!quiet_s && ca.hist && vblk == 0u && threadIdx.x == 0) scal->spec.flags = 0u;
            }
            if (quiet_s) {
                if (zs.count && threadIdx.x == 0) {  // (a quiet exit is a skip: both counters)
                    unsigned long long stands_for = 1ull;
                    if constexpr (THIN) {  // (the blocks of this workgroup that hold particles: what the one-block form would have counted)
                        stands_for = 0ull;
                        for (uint32_t v = vblk; v < vgrid; v += gridDim.x) stands_for += xcd_map(v, vgrid, K.rev, K.xcd_shift) * 256u < n ? 1ull : 0ull;
                    }
                    atomicAdd(&scal->stripe[blockIdx.x % STRIPES].zs_skipped, stands_for);
                    atomicAdd(&scal->stripe[blockIdx.x % STRIPES].zs_quiet, stands_for);
                }
                if constexpr (THIN && INV_DT) {  // the correction is the identity: the producer's count stands, and so do its flags
                    if (ca.hist && vblk == 0u && threadIdx.x == 0) {
                        const uint32_t f = scal->spec.flags;
                        if (f) {
                            atomicOr(&scal->flags, f);
                            scal->spec.flags = 0u;
                        }
                    }
                }
                verdict();
                if constexpr (THIN) SPHX_CORRECT_LEAVE(true);  // (the sums are the producer's: nb_tail<2, TAKE>, k_compute_error<.., TAKE>)
                float2 pnew = make_float2(0.0f, 0.0f);
                DirAhead ahead{0xFFFFFFFFu, EMPTY};
                if (i < n) {
                    if (INV_DT) {
                        if (ca.hist) {
                            uint32_t cx0, cy0;
                            cell_of(K, pi, cx0, cy0);
                            ahead = dir_ahead(ca.g, cx0, cy0);
                        }
                        pnew = make_float2(pi.x + vi.x * dt, pi.y + vi.y * dt);  // dfsph.rs:499-510, as the skip's exit below
                    }
                    store_cold(&warm[i], warm_i + ki, K.nt_cold);  // dfsph.rs:142 / :296
                }
                if (INV_DT)
                    if (ca.hist) count_cell(K, ca.g, i < n, i, pnew, ca.hist, ca.cidx, 1u, scal, ahead);
                SPHX_CORRECT_LEAVE(true);
            }
        }
    }
    // zero-correction skip, 1: the flag words of the wavefronts that overlap the window [lw0, lw0 + lwlen) of nb_head — contiguous, at
    // most nine — requested here (scalar loads), looked at behind the head's loads
    bool zs_try = false;
    uint32_t zf[9] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if constexpr (ZS) {
        const uint32_t b0 = blk0 * 256u;
        // (scalar conditions; inv_dt may have come from device memory: the host cannot vouch for it)
        if (zs.knz && b0 < n && (!INV_DT || (inv_dt > 0.0f && inv_dt <= 3.402823466e38f))) {
            zs_try = true;
            const uint32_t lw0 = b0 > LIST_HALO ? b0 - LIST_HALO : 0u, lwend = min(b0 + 256u + LIST_HALO, n);
            const uint32_t f0 = lw0 >> 6, f1 = (lwend - 1u) >> 6;
            static_assert((LIST_WIN + 62u) / 64u + 1u <= 9u, "flag words of a window");
#pragma unroll
            for (uint32_t u = 0; u < 9u; ++u) zf[u] = zs.knz[min(f0 + u, f1)];
        }
    }
    Loaded LA = load_head(blk0);
    if constexpr (ZS) {
        if (zs_try) {
            if (zf[0] | zf[1] | zf[2] | zf[3] | zf[4] | zf[5] | zf[6] | zf[7] | zf[8]) {
                if (zs.count && threadIdx.x == 0) atomicAdd(&scal->stripe[blockIdx.x % STRIPES].zs_window, 1ull);
            } else {
                // 2. a wavefront in the wide format gathers from anywhere: today's path.  3. the fluid records behind the lines of the
                // out-of-window tables (every line in use belongs to some list entry of its wavefront; boundary records carry k = 0).
                // The lines and the wavefront's word are the head's; what the skip needs of the own particle rides with the flags.
                const NbHead& h = LA.h;
                const uint32_t lane = threadIdx.x & 63u;
                const uint32_t i = LA.i, ic = min(i, n - 1u);
                const float ki = kbuf[ic];
                const float2 pi = INV_DT ? gat(posA, ic) : make_float2(0.0f, 0.0f);
                static_assert(WAVE_REMOTE == 128, "two halves of 64 lines");
                uint32_t g1 = h.g[1];
                if (nb.lazy_hi && h.R > 64u) g1 = h.rtab[lane + 64u];  // (nb_head leaves the upper half to nb_head_late)
                uint32_t veto = h.wide ? 1u : 0u;
                if (lane < h.R && h.g[0] < soff) veto |= zs.knz[h.g[0] >> 6];
                if (lane + 64u < h.R && g1 < soff) veto |= zs.knz[g1 >> 6];
                if (__syncthreads_or((int)veto)) {
                    if (zs.count && threadIdx.x == 0) atomicAdd(&scal->stripe[blockIdx.x % STRIPES].zs_remote, 1ull);
                } else {
                    // 4. skip: no staging, no walk, no velocity store
                    if (zs.count && threadIdx.x == 0) atomicAdd(&scal->stripe[blockIdx.x % STRIPES].zs_skipped, 1ull);
                    verdict();
                    float2 pnew = make_float2(0.0f, 0.0f);
                    DirAhead ahead{0xFFFFFFFFu, EMPTY};
                    if (i < n) {
                        if (INV_DT) {
                            if (ca.hist) {
                                uint32_t cx0, cy0;
                                cell_of(K, pi, cx0, cy0);
                                ahead = dir_ahead(ca.g, cx0, cy0);
                            }
                            // dfsph.rs:499-510 on the velocity the walk would have stored back
                            pnew = make_float2(pi.x + LA.pvi.z * dt, pi.y + LA.pvi.w * dt);
                        }
                        store_cold(&warm[i], LA.warm_i + ki, K.nt_cold);  // dfsph.rs:142 / :296
                    }
                    if (INV_DT)
                        if (ca.hist) {
                            // (THIN: the position is the speculated one again — the recount finds the cell it has, touches no
                            // count and raises the flags the dropped word held for this particle)
                            if constexpr (THIN)
                                recount_cell(K, ca.g, i < n, i, pnew, ca.hist, ca.cidx, scal, ahead, zs.count);
                            else
                                count_cell(K, ca.g, i < n, i, pnew, ca.hist, ca.cidx, 1u, scal, ahead);
                        }
                    SPHX_CORRECT_LEAVE(false);
                }
            }
        }
    }
    load_stage(LA);
    if (LA.h.lwlen) nb_stage_store(LA.h, LA.st, store_rec);
    verdict();
    auto process = [&](const Loaded& L) {
    const uint32_t i = L.i, blk = L.blk;
    const NbHead& h = L.h;
    float4 pvi = L.pvi;
    const float warm_i = L.warm_i;
    const uint32_t id_i = L.id_i;
    DirAhead ahead = L.ahead;
    (void)blk;
    (void)id_i;
    __syncthreads();
    if (i < n) {
        const float2 pi = h.wide ? gat(posA, i) : rec.vec<0>((i - h.lw0) * 4u);
        pvi.x = pi.x, pvi.y = pi.y;
        if (!WARM && INV_DT && ca.hist) {
            // the cell count at the end of this kernel needs the directory entry of the particle's block: requested now, in front of the
            // walk, for the block the particle is in BEFORE it moves (a particle rarely changes its 64 x 64 block)
            uint32_t cx0, cy0;
            cell_of(K, pi, cx0, cy0);
            ahead = dir_ahead(ca.g, cx0, cy0);
        }
    }
    (void)ahead;
    float2 pnew = make_float2(0.0f, 0.0f);
    if (i < n) {
        const uint32_t ct = h.ct;
        float ki;
        float2 ri;
        ri = make_float2(pvi.x, pvi.y);
        if (WARM)
            ki = 0.5f * fmaxf(warm_i, lim);
        else
            ki = h.wide ? kbuf[i] : rec.scal<0>((i - h.lw0) * 4u);
        float dx = 0.0f, dy = 0.0f;
        struct Rec {
            float2 p;
            float w;
        };
        auto walk = [&](auto fast) {
            auto consume = [&](const Rec& q, uint32_t) {
                const float2 g = wendland_grad<decltype(fast)::value>(K, ri, q.p);
                // (ki + kj), dfsph.rs:151 / :184 / :305 / :335; static neighbours: kj = 0 (staged so), i.e. ki alone, dfsph.rs:156 / :188 / :309 / :339
                const float kj = WARM ? 0.5f * fmaxf(q.w, lim) : q.w;
                const float s = ki + kj;
                dx = dx + s * g.x;
                dy = dy + s * g.y;
            };
            nb_traverse(
                h, ct, [&](uint32_t o) { return Rec{rec.vec<0>(o), rec.scal<0>(o)}; },
                [&](uint32_t g) {
                    const float w = gat(wsrc, g < soff ? g : i);
                    return Rec{gat(posA, g), g < soff ? w : 0.0f};
                },
                consume);
        };
        if (K.q_noclamp)  // (kernel argument: a scalar branch; sqrt_dist)
            walk(std::true_type{});
        else
            walk(std::false_type{});
        float2 o;
        if (INV_DT) {
            o.x = pvi.z - (inv_dt * dx) * K.mass;  // dfsph.rs:159 / :191
            o.y = pvi.w - (inv_dt * dy) * K.mass;
        } else {
            o.x = pvi.z - dx * K.mass;  // dfsph.rs:312 / :342
            o.y = pvi.w - dy * K.mass;
        }
        vel[i] = o;
        if (!WARM) {  // dfsph.rs:142 / :296 (read again by the next step's loop: Consts::nt_cold)
            store_cold(&warm[i], warm_i + ki, K.nt_cold);
        }
        pnew = make_float2(pvi.x + o.x * dt, pvi.y + o.y * dt);  // dfsph.rs:499-510, the operations of k_key_count<true>
    }
    if (!WARM && INV_DT)
        if (ca.hist) {
            if (TILE) {  // k_tile_count's and k_tile_pack's verdicts, from the position in registers
                __shared__ uint32_t wc[4][MAX_TILE_PEERS];
                const uint32_t m = i < n ? tile_send_mask(K, tc.rect, tc.n, tc.halo, make_float4(pnew.x, pnew.y, 0.0f, 0.0f), id_i) : 0u;
                for (uint32_t k = 0; k < tc.n; ++k) {
                    const uint32_t c = (uint32_t)__popcll(__ballot((m >> k) & 1u));
                    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6][k] = c;
                }
                if (i < n) {
                    // what the tile keeps: its own particles (owner bit) that are still inside the rectangle grown by the ghost band;
                    // last step's ghosts and whatever left the band get no cell (k_tile_pack marked those with a NaN position)
                    uint32_t cx, cy;
                    cell_of(K, pnew, cx, cy);
                    if (!((id_i >> 31) != 0 && pnew.x == pnew.x && rect_has(K.tile, cx, cy, tc.halo))) pnew.x = __uint_as_float(0x7FC00000u);
                }
                count_cell(K, ca.g, i < n, i, pnew, ca.hist, ca.cidx, 1u, scal, ahead);
                // (the send counts last: the barrier they need then only holds back wavefronts that have nothing left to do; a tile
                // without neighbours has none to write)
                if (tc.n) {
                    __syncthreads();
                    if (threadIdx.x < 64) {
                        const uint32_t v = threadIdx.x < tc.n ? wc[0][threadIdx.x] + wc[1][threadIdx.x] + wc[2][threadIdx.x] + wc[3][threadIdx.x] : 0u;
                        if (threadIdx.x < MAX_TILE_PEERS) tc.blk[(size_t)blk * MAX_TILE_PEERS + threadIdx.x] = v;
                        const unsigned long long sends = __ballot(v != 0u);
                        if (threadIdx.x == 0) tc.any[blk] = sends ? 1u : 0u;
                    }
                }
                return;
            }
            if constexpr (THIN)  // (the producer has counted p + v* dt: move the particles whose corrected velocity takes them elsewhere)
                recount_cell(K, ca.g, i < n, i, pnew, ca.hist, ca.cidx, scal, ahead, zs.count);
            else
                count_cell(K, ca.g, i < n, i, pnew, ca.hist, ca.cidx, 1u, scal, ahead);  // every density correction counts
        }
    };
    process(LA);
