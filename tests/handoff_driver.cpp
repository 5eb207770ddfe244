// Stand-alone driver for the hand-off records of the host step path (yasph2d_amd/csrc/sphx_handoff.hpp): plain C++, compiled by
// tests/test_handoff_host.py with the address and undefined-behaviour sanitizers (any report aborts the program).
//   handoff_driver build | count [depth]      (depth: longest sequence, default 6)
// Each half restates, as the MODEL, the loose sphx_ctx members a record replaced and every statement that touched them, literally
// as sphx_launch.inc / sphx_state.inc had them; next to it stands the same host code written with the record.  Both are driven
// through every sequence of the events below up to the given length, and after every event everything a consumer is told is compared:
// which launches are queued or left out, which instantiation, what a test answers, the error returns.  The records' internal state is
// not compared.  Prints "ok <sequences> <comparisons>" and returns 0, or the first sequence whose answers differ and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sphx_handoff.hpp"

using namespace sphx;

struct Ans {  // what one event told its consumers
    int v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool operator==(const Ans& o) const { return std::memcmp(v, o.v, sizeof(v)) == 0; }
};
enum { OK = 0, ERR_INVALID = -1, ERR_REGRID_DIV_WARM = -2, ERR_REGRID_WARM_DENSITY = -3, ERR_REGRID_DIV_ITER = -4 };

// =====================================================================================================================
// 1. BuildHandoff against div_error_fused, div_warm_fused, div_knz_fused, div_mark_tag, div_warm_taken
// =====================================================================================================================
namespace build {

enum Kind { PLAIN, FUSE, FUSE_DIV, FUSE_WARM };  // k_neighbor_build<0 .. 3>
struct Shared {                                  // context members both forms read and advance alike
    uint32_t seq = 0, res_seq = 0;
};

struct Model : Shared {
    bool div_error_fused = false, div_warm_fused = false, div_knz_fused = false, div_warm_taken = false;
    uint32_t div_mark_tag = 0;

    // update_neighborhood: v[0] = the TAKE instantiation was launched
    Ans neighbor_build(uint32_t n, Kind kind, bool flags, bool take_over) {
        Ans a;
        if (n) {
            div_error_fused = false;
            div_warm_fused = false;
            div_knz_fused = false;
            div_warm_taken = false;
            if (kind == FUSE_WARM) {
                div_warm_fused = true;
            } else if (kind == FUSE_DIV) {
                div_knz_fused = flags;
                div_mark_tag = res_seq + 1u;
                if (flags && take_over) div_warm_taken = true;
                a.v[0] = div_warm_taken;
                div_error_fused = true;
            }
        }
        return a;
    }
    // enqueue_iteration: v[0] warm start launched, v[1] compute_error launched, v[2] the correction gets flags, v[3] ... is told warm_taken
    // (flags exist; a take-over decided by the iteration itself is not the record's business: left out on both sides)
    Ans enqueue_iteration(bool out_warm, bool divergence, bool first, bool warm) {
        Ans a;
        if (out_warm && first) {
            if (warm && divergence && div_warm_fused)
                div_warm_fused = false;
            else if (warm)
                a.v[0] = 1;
        }
        ++seq;
        const uint32_t rseq = ++res_seq;
        bool knz = true, warm_taken = false;
        if (divergence && first && div_error_fused) {
            div_error_fused = false;
            if (!div_knz_fused || div_mark_tag != rseq) knz = false;
            warm_taken = knz && div_warm_taken;
        } else {
            a.v[1] = 1;
        }
        div_warm_taken = false;
        a.v[2] = knz;
        a.v[3] = warm_taken;
        return a;
    }
    // sphx_sub_warmstart: v[0] the return, v[1] warm start launched
    Ans sub_warmstart(bool divergence) {
        Ans a;
        if (div_error_fused) return a.v[0] = ERR_REGRID_DIV_WARM, a;
        if (div_warm_fused) {
            div_warm_fused = false;
            if (!divergence) return a.v[0] = ERR_REGRID_WARM_DENSITY, a;
            return a;
        }
        a.v[1] = 1;
        return a;
    }
    // sub_iteration_impl: v[4] the return, v[5] / v[6] the sequence numbers after it, the rest as enqueue_iteration
    Ans sub_iteration(bool divergence, bool first) {
        Ans a;
        div_warm_fused = false;
        if (div_error_fused && !(divergence && first)) {
            div_error_fused = false;
            ++seq, ++res_seq;
            a.v[4] = ERR_REGRID_DIV_ITER;
        } else {
            a = enqueue_iteration(false, divergence, first, false);
        }
        a.v[5] = (int)seq, a.v[6] = (int)res_seq;
        return a;
    }
    void broken() { div_error_fused = div_warm_fused = false; }      // sphx_step_finish's failure path
    void state_load() { div_error_fused = div_warm_fused = false; }  // sphx_state_load
};

struct Branch : Shared {
    BuildHandoff handoff;

    Ans neighbor_build(uint32_t n, Kind kind, bool flags, bool take_over) {
        Ans a;
        if (n) {
            handoff.clear();
            if (kind == FUSE_WARM) {
                handoff = BuildHandoff::warm_applied();
            } else if (kind == FUSE_DIV) {
                const uint32_t tag = res_seq + 1u;
                const bool take = flags && take_over;
                a.v[0] = take;
                handoff = BuildHandoff::first_errors(flags, tag, take);
            }
        }
        return a;
    }
    Ans enqueue_iteration(bool out_warm, bool divergence, bool first, bool warm) {
        Ans a;
        if (out_warm && first) {
            if (warm && !(divergence && handoff.take_warm())) a.v[0] = 1;
        }
        ++seq;
        const uint32_t rseq = ++res_seq;
        bool knz = true, warm_taken = false;
        const BuildHandoff::Taken built = handoff.take_first_errors(divergence && first, rseq);
        if (built.fused) {
            if (!built.flags_usable) knz = false;
            warm_taken = knz && built.warm_taken;
        } else {
            a.v[1] = 1;
        }
        a.v[2] = knz;
        a.v[3] = warm_taken;
        return a;
    }
    Ans sub_warmstart(bool divergence) {
        Ans a;
        if (handoff.first_errors_pending()) return a.v[0] = ERR_REGRID_DIV_WARM, a;
        if (handoff.take_warm()) return a.v[0] = divergence ? OK : ERR_REGRID_WARM_DENSITY, a;
        a.v[1] = 1;
        return a;
    }
    Ans sub_iteration(bool divergence, bool first) {
        Ans a;
        const bool refused = handoff.first_errors_pending() && !(divergence && first);
        if (refused || !handoff.first_errors_pending()) handoff.clear();
        if (refused) {
            ++seq, ++res_seq;
            a.v[4] = ERR_REGRID_DIV_ITER;
        } else {
            a = enqueue_iteration(false, divergence, first, false);
        }
        a.v[5] = (int)seq, a.v[6] = (int)res_seq;
        return a;
    }
    void broken() { handoff.clear(); }
    void state_load() { handoff.clear(); }
};

// builds: the four kinds, FUSE_DIV with and without flags and take-over, and one over zero particles; the single context's
// iterations (first with and without a warm start, non-first; both loops); the tile sub-steps; the two resets
// (an alphabet of 18 keeps depth 6 within a few seconds; left out as repeats of a neighbour: a take-over hint without flags, a
// warm-start build over zero particles, the density loop's non-first iteration, the tile's first density iteration)
constexpr int EVENTS = 18;
template <class S>
Ans apply(S& s, int e) {
    switch (e) {
        case 0: return s.neighbor_build(5, PLAIN, false, false);
        case 1: return s.neighbor_build(5, FUSE, false, false);
        case 2: return s.neighbor_build(5, FUSE_WARM, false, false);
        case 3: return s.neighbor_build(5, FUSE_DIV, false, false);
        case 4: return s.neighbor_build(5, FUSE_DIV, true, false);
        case 5: return s.neighbor_build(5, FUSE_DIV, true, true);
        case 6: return s.neighbor_build(0, FUSE_DIV, true, true);
        case 7: return s.enqueue_iteration(true, true, true, true);
        case 8: return s.enqueue_iteration(true, true, true, false);
        case 9: return s.enqueue_iteration(true, true, false, true);
        case 10: return s.enqueue_iteration(true, false, true, true);
        case 11: return s.enqueue_iteration(true, false, true, false);
        case 12: return s.sub_iteration(true, true);
        case 13: return s.sub_iteration(true, false);
        case 14: return s.sub_warmstart(true);
        case 15: return s.sub_warmstart(false);
        case 16: return s.broken(), Ans{};
        default: return s.state_load(), Ans{};
    }
}
using M = Model;
using B = Branch;
}  // namespace build

// =====================================================================================================================
// 2. PendingCount against count_done, count_n, count_from_class, tile_class_done, tile_class_n, tile_class_dt_bits
// =====================================================================================================================
namespace count {

struct Shared {  // context members both forms read and advance alike
    bool tile_mode = false;
    uint32_t N = 5;
    float tile_pending_dt = 0.0f;
    uint32_t tile_pending_n = 0;
    bool tile_fix_owner = false;
    int wipes = 0, advects = 0;  // hipMemsetAsync of gdyn.hist / launches of flush_pending_advect so far
};
static uint32_t bits_of(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// The entry points, written once over the few statements (`P`) that touch the members or the record.
template <class P>
struct Host : Shared, P {
    void flush_pending_advect() {
        P::drop_class_count(*this);
        if (!(tile_pending_dt > 0.0f)) return;
        tile_pending_dt = 0.0f;
        tile_pending_n = 0;
        tile_fix_owner = false;
        advects += 1;
    }
    // enqueue_context_iteration + enqueue_iteration of a density loop inside sphx_step_finish: v[0] counts, v[1] clear_hist handed over
    Ans context_correction(bool device_next) {
        Ans a;
        const bool counts = !tile_mode;
        const bool drop_count = counts && !device_next;
        if (counts && !drop_count) a.v[1] = P::live(*this);
        if (drop_count) P::drop_fused_count(*this);
        if (drop_count) P::drop_fused_count(*this);
        if (counts) P::made_by_correction(*this, N);
        a.v[0] = counts;
        return merge(a);
    }
    // sub_iteration_impl (classify: every condition of the classifying correction holds): v[0] classifies
    Ans sub_iteration(bool classify, float dt) {
        Ans a;
        P::sub_step_enter(*this);
        if (!N) return merge(a);
        const bool drop_count = classify && tile_mode;
        if (drop_count) P::drop_fused_count(*this);
        if (drop_count) P::drop_fused_count(*this);
        if (drop_count) P::made_by_classifier(*this, N, dt);
        a.v[0] = drop_count;
        return merge(a);
    }
    // tile_pack_impl (directory_stable: the conditions of the fused count): v[0] the return, v[1] band pack, v[2] counts, v[3] defers
    Ans tile_pack(float advect_dt, bool directory_stable) {
        Ans a;
        if (!tile_mode) return a.v[0] = ERR_INVALID, merge(a);
        const uint32_t n = N;
        if (!n) return merge(a);
        if (P::take_over(*this, n, advect_dt)) {
            a.v[1] = 1;
            tile_pending_dt = advect_dt;
            tile_pending_n = n;
            tile_fix_owner = true;
            return merge(a);
        }
        P::pack_goes_on(*this);
        flush_pending_advect();
        if (directory_stable) {
            P::drop_fused_count(*this);
            P::made_by_pack(*this, n);
            a.v[2] = 1;
        }
        const bool defer = advect_dt > 0 && directory_stable;
        if (defer) {
            tile_pending_dt = advect_dt;
            tile_pending_n = n;
        }
        a.v[3] = defer;
        return merge(a);
    }
    // sphx_tile_count_kept: v[0] the return, v[1] k_key_count launched
    Ans tile_count_kept(bool directory_stable) {
        Ans a;
        if (!tile_mode) return a.v[0] = ERR_INVALID, merge(a);
        P::bar(*this);
        const uint32_t n = N;
        if (!n || !directory_stable) return merge(a);
        P::drop_class_count(*this);
        if (P::is_for(*this, n)) return merge(a);
        flush_pending_advect();
        P::drop_fused_count(*this);
        a.v[1] = 1;
        P::made_by_pack(*this, n);
        return merge(a);
    }
    // sphx_tile_configure_rect / sphx_tile_apply_n (two arrivals) / the start of sphx_tile_upload
    Ans tile_configure() {
        P::bar(*this);
        tile_mode = true;
        return merge(Ans{});
    }
    Ans tile_apply() {
        Ans a;
        if (!tile_mode) return a.v[0] = ERR_INVALID, merge(a);
        P::bar(*this);
        N += 2;
        return merge(a);
    }
    // update_neighborhood + build_grid of the dynamic grid.  v[0] the gather advects what the pack deferred, v[1] counted,
    // v[2] partial, v[3] first, v[4] k_key_count launched
    Ans neighbor_build(float advect_dt) {
        Ans a;
        P::drop_class_count(*this);
        if (tile_pending_dt > 0.0f) {
            if (tile_mode && advect_dt == 0.0f && P::is_for(*this, tile_pending_n) && tile_pending_n <= N) {
                a.v[0] = 1;
                tile_pending_dt = 0.0f;
                tile_pending_n = 0;
                tile_fix_owner = false;
            } else {
                flush_pending_advect();
            }
        }
        const uint32_t n = N;
        const bool tile_n = tile_mode;
        uint32_t first = 0;
        bool counted = false, partial = false;
        P::build_grid_dynamic(*this, n, advect_dt, tile_n, &counted, &partial, &first);
        a.v[1] = counted, a.v[2] = partial, a.v[3] = (int)first, a.v[4] = n > first && !counted;
        return merge(a);
    }
    Ans set_directory() { return P::new_directory(*this), merge(Ans{}); }        // (clear_histograms — sphx_upload, sphx_state_load — says the same)
    Ans drop_fused_count() { return P::drop_fused_count(*this), merge(Ans{}); }  // sphx_append / _remove, a refused sphx_step_finish, the boundary's build
    Ans merge(Ans a) const {
        a.v[6] = wipes, a.v[7] = advects;
        return a;
    }
};

struct ModelPolicy {
    bool count_done = false, count_from_class = false, tile_class_done = false;
    uint32_t count_n = 0, tile_class_n = 0, tile_class_dt_bits = 0;
    template <class H>
    static void drop_fused_count(H& c) {
        if (!c.count_done) return;
        c.count_done = false;
        c.wipes += 1;
    }
    template <class H>
    static void drop_class_count(H& c) {
        if (!c.count_from_class) return;
        c.count_from_class = false;
        c.tile_class_done = false;
        drop_fused_count(c);
    }
    template <class H>
    static void new_directory(H& c) {
        c.count_done = false;
    }
    template <class H>
    static void sub_step_enter(H& c) {
        c.tile_class_done = false;
        c.flush_pending_advect();
    }
    template <class H>
    static void bar(H& c) {
        c.tile_class_done = false;
    }
    template <class H>
    static void pack_goes_on(H& c) {
        c.tile_class_done = false;
    }
    template <class H>
    static bool live(const H& c) {
        return c.count_done;
    }
    template <class H>
    static bool is_for(const H& c, uint32_t n) {
        return c.count_done && c.count_n == n;
    }
    template <class H>
    static void made_by_correction(H& c, uint32_t n) {
        c.count_done = true;
        c.count_n = n;
    }
    template <class H>
    static void made_by_pack(H& c, uint32_t n) {
        c.count_done = true;
        c.count_n = n;
    }
    template <class H>
    static void made_by_classifier(H& c, uint32_t n, float dt) {
        c.count_done = true;  // (enqueue_iteration)
        c.count_n = n;
        c.tile_class_done = true;  // (sub_iteration_impl, behind it)
        c.count_from_class = true;
        c.tile_class_n = n;
        std::memcpy(&c.tile_class_dt_bits, &dt, 4);
    }
    template <class H>
    static bool take_over(H& c, uint32_t n, float advect_dt) {
        const uint32_t dt_bits = bits_of(advect_dt);
        if (c.tile_class_done && c.count_done && c.count_n == n && c.tile_class_n == n && advect_dt > 0 && dt_bits == c.tile_class_dt_bits &&
            !(c.tile_pending_dt > 0.0f)) {
            c.tile_class_done = false;
            c.count_from_class = false;
            return true;
        }
        return false;
    }
    template <class H>
    static void build_grid_dynamic(H& c, uint32_t n, float advect_dt, bool tile_n, bool* out_counted, bool* out_partial, uint32_t* out_first) {
        const bool counted = c.count_done && advect_dt > 0 && c.count_n == n && !tile_n;
        const bool partial = c.count_done && tile_n && advect_dt == 0.0f && c.count_n <= n && !counted;
        uint32_t first = 0;
        if (counted || partial) {
            c.count_done = false;
            if (partial) first = c.count_n;
        } else {
            drop_fused_count(c);
        }
        *out_counted = counted, *out_partial = partial, *out_first = first;
    }
};

struct BranchPolicy {
    PendingCount pending;
    template <class H>
    static void drop_fused_count(H& c) {
        if (c.pending.drop()) c.wipes += 1;
    }
    template <class H>
    static void drop_class_count(H& c) {
        if (c.pending.drop_if_from_classifier()) c.wipes += 1;
    }
    template <class H>
    static void new_directory(H& c) {
        c.pending.forget();
    }
    template <class H>
    static void sub_step_enter(H& c) {
        c.flush_pending_advect();
    }
    template <class H>
    static void bar(H& c) {
        c.pending.bar_take_over();
    }
    template <class H>
    static void pack_goes_on(H&) {}
    template <class H>
    static bool live(const H& c) {
        return c.pending.live();
    }
    template <class H>
    static bool is_for(const H& c, uint32_t n) {
        return c.pending.is_for(n);
    }
    template <class H>
    static void made_by_correction(H& c, uint32_t n) {
        c.pending.made_by_correction(n);
    }
    template <class H>
    static void made_by_pack(H& c, uint32_t n) {
        c.pending.made_by_pack(n);
    }
    template <class H>
    static void made_by_classifier(H& c, uint32_t n, float dt) {
        c.pending.made_by_classifier(n, dt);
    }
    template <class H>
    static bool take_over(H& c, uint32_t n, float advect_dt) {
        return advect_dt > 0 && !(c.tile_pending_dt > 0.0f) && c.pending.take_over_class(n, advect_dt);
    }
    template <class H>
    static void build_grid_dynamic(H& c, uint32_t n, float advect_dt, bool tile_n, bool* out_counted, bool* out_partial, uint32_t* out_first) {
        const bool counted = advect_dt > 0 && !tile_n && c.pending.is_for(n);
        const bool partial = tile_n && advect_dt == 0.0f && !counted && c.pending.is_for_first_of(n);
        const uint32_t first = partial ? c.pending.n() : 0u;
        if (counted || partial)
            c.pending.forget();
        else
            drop_fused_count(c);
        *out_counted = counted, *out_partial = partial, *out_first = first;
    }
};

constexpr float DT_A = 0.001f, DT_B = 0.002f;
// (an alphabet of 16 keeps depth 6 within a few seconds; left out as repeats of a neighbour: a classifying correction with the other
// dt — the packs differ in theirs —, the boundary's build, which is a bare drop_fused_count, and clear_histograms, which tells the
// record what a new directory tells it)
constexpr int EVENTS = 16;
template <class S>
Ans apply(S& s, int e) {
    switch (e) {
        case 0: return s.context_correction(false);  // the first of a loop, or any of a host-run loop
        case 1: return s.context_correction(true);   // a later one of a device-run loop
        case 2: return s.sub_iteration(true, DT_A);
        case 3: return s.sub_iteration(false, DT_A);  // also sphx_sub_predict, _warmstart, _nonpressure, _advect: the preamble alone
        case 4: return s.tile_pack(DT_A, true);
        case 5: return s.tile_pack(DT_B, true);
        case 6: return s.tile_pack(0.0f, true);
        case 7: return s.tile_pack(DT_A, false);
        case 8: return s.tile_count_kept(true);
        case 9: return s.tile_count_kept(false);
        case 10: return s.tile_configure();
        case 11: return s.tile_apply();
        case 12: return s.neighbor_build(DT_A);  // the step's own build (a tile never asks for one)
        case 13: return s.neighbor_build(0.0f);  // a tile's re-grid, the warm-up build of a single context
        case 14: return s.set_directory();
        default: return s.drop_fused_count();
    }
}
using M = Host<ModelPolicy>;
using B = Host<BranchPolicy>;
}  // namespace count

// ---- every sequence up to `depth` events, depth first: a prefix is run once ----------------------------------------
static long g_sequences = 0, g_checks = 0;
static int g_path[16];

template <class M, class B, int EVENTS, Ans (*AM)(M&, int), Ans (*AB)(B&, int)>
static void walk(const M& m, const B& b, int len, int depth) {
    for (int e = 0; e < EVENTS; ++e) {
        M m2 = m;
        B b2 = b;
        const Ans am = AM(m2, e), ab = AB(b2, e);
        g_path[len] = e;
        ++g_checks;
        if (!(am == ab)) {
            std::printf("FAILED: the answers differ after the events");
            for (int k = 0; k <= len; ++k) std::printf(" %d", g_path[k]);
            std::printf("\n  model :");
            for (int v : am.v) std::printf(" %d", v);
            std::printf("\n  record:");
            for (int v : ab.v) std::printf(" %d", v);
            std::printf("\n");
            std::exit(1);
        }
        ++g_sequences;
        if (len + 1 < depth) walk<M, B, EVENTS, AM, AB>(m2, b2, len + 1, depth);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) return std::printf("usage: handoff_driver build | count [depth]\n"), 2;
    const int depth = argc > 2 ? std::atoi(argv[2]) : 6;
    if (depth < 1 || depth > 16) return std::printf("depth must be 1 .. 16\n"), 2;
    if (!std::strcmp(argv[1], "build")) {
        walk<build::M, build::B, build::EVENTS, build::apply<build::M>, build::apply<build::B>>(build::M{}, build::B{}, 0, depth);
    } else if (!std::strcmp(argv[1], "count")) {
        for (int tile = 0; tile < 2; ++tile) {  // a context is a tile for good once configured: both starts get the full depth
            count::M m;
            count::B b;
            m.tile_mode = b.tile_mode = tile != 0;
            walk<count::M, count::B, count::EVENTS, count::apply<count::M>, count::apply<count::B>>(m, b, 0, depth);
        }
    } else {
        return std::printf("unknown check %s\n", argv[1]), 2;
    }
    std::printf("ok %ld %ld\n", g_sequences, g_checks);
    return 0;
}
