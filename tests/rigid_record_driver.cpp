// Stand-alone driver for the rigid-motion record of the host step path (sphx::VelMarks, yasph2d_amd/csrc/sphx_handoff.hpp): plain
// C++, compiled by tests/test_rigid_record_host.py with the address and undefined-behaviour sanitizers (any report aborts).
//   rigid_record_driver [depth]      (depth: longest sequence, default 6)
// The MODEL is the velocity array itself, reduced to what the identity needs: `mixed` — some velocity's bits differ from vel[0]'s —
// and the two mark words as the kernels write them (one stripe stands for the 32: the consumer ORs them).  Next to it stands the host
// code of sphx_launch.inc written with the record.  Both are driven through every sequence of the events below up to the given
// length; at every run-ahead launch the driver checks
//   soundness: a launch that would leave through the rigid exit (record usable, no mark under its tags) finds the array uniform;
//   liveness:  a gather over a uniform array, thin corrections without factors behind it at most, then the launch: the rigid exit.
// Prints "ok <sequences> <launches checked> <rigid exits>" and returns 0, or the first offending sequence and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "sphx_handoff.hpp"

using namespace sphx;

enum Event {
    GATHER_MARKS,        // build_grid, the fluid build inside a single context's step (GatherArgs::vmix_tag != 0)
    GATHER_PLAIN,        // build_grid of the dynamic grid without marks (a tile, sphx_update_neighborhood, the switch off)
    THIN_QUIET,          // k_correct_thin, every k +-0: no velocity is written, no knz mark
    THIN_MARKED,         // k_correct_thin with a factor: its producer stored the iteration's knz mark, the walk writes velocities
    CORRECT_QUIET,       // a correction in another form, every k +-0
    CORRECT_WRITES,      // a correction in another form that changes velocities (with or without a mark of its own)
    BUILD_WARM,          // k_neighbor_build<3>: the warm start applied behind the gather
    WARMSTART,           // launch_warmstart
    PREDICT,             // k_predict / compute_density_error with the prediction: v + a dt, uniform iff it was (a is uniform then)
    UPLOAD_MIXED,        // sphx_upload / sphx_append / sphx_remove / sphx_state_load / lists_went_stale with other velocities
    FAILED_CALL,         // sphx_ctx::fail, sphx_step_finish's broken(): the arrays are mid-step
    RUN_AHEAD,           // enqueue_run_ahead: the taking call
    N_EVENTS
};
static const char* const NAMES[N_EVENTS] = {"gather+marks", "gather",   "thin quiet", "thin marked", "correct quiet", "correct writes",
                                            "build<3>",     "warmstart", "predict",    "upload",      "failed call",   "run-ahead"};

struct World {
    // the device
    bool mixed = false;  // starts uniform (all zero), like an upload without velocities
    uint32_t vmix_mark = 0, knz_mark = 0;
    // the host
    uint32_t gather_seq = 0, res_seq = 0;
    VelMarks rec;
    // liveness bookkeeping: a marked gather over a uniform array, nothing but quiet thin corrections since
    bool clean_run = false;
};

struct Verdict {
    bool launched_judged, rigid_exit;
};

static Verdict apply(World& w, Event e) {
    Verdict v{false, false};
    switch (e) {
    case GATHER_MARKS:
        w.rec.wrote();
        if (++w.gather_seq == 0) w.gather_seq = 1;
        if (w.mixed) w.vmix_mark = w.gather_seq;  // the gather's ballot and store
        w.rec.made(w.gather_seq);
        w.clean_run = !w.mixed;
        break;
    case GATHER_PLAIN:
        w.rec.wrote();
        w.clean_run = false;
        break;
    case THIN_QUIET:
        w.rec.thin(++w.res_seq);
        if (!w.rec.valid) w.clean_run = false;  // (a second thin correction voids: one knz tag travels)
        break;
    case THIN_MARKED:
        w.knz_mark = ++w.res_seq;  // knz_store of the iteration's producer
        w.rec.thin(w.res_seq);
        w.mixed = true;
        w.clean_run = false;
        break;
    case CORRECT_QUIET:
        ++w.res_seq;
        w.rec.wrote();
        w.clean_run = false;
        break;
    case CORRECT_WRITES:
        ++w.res_seq;
        w.rec.wrote();
        w.mixed = true;
        w.clean_run = false;
        break;
    case BUILD_WARM:
    case WARMSTART:
        w.rec.wrote();
        w.mixed = true;
        w.clean_run = false;
        break;
    case PREDICT:
        w.rec.wrote();
        w.clean_run = false;
        break;
    case UPLOAD_MIXED:
    case FAILED_CALL:
        w.rec.wrote();
        w.mixed = true;
        w.clean_run = false;
        break;
    case RUN_AHEAD: {
        const VelMarks::Taken t = w.rec.take();
        if (t.usable) {
            // rigid_marked(): the 32 vmix words under the gather's tag, the 32 knz words under the thin correction's
            const bool marked = w.vmix_mark == t.tag || (t.check_knz && w.knz_mark == t.knz_tag);
            v.launched_judged = true;
            v.rigid_exit = !marked;
        }
        break;
    }
    default:
        break;
    }
    return v;
}

int main(int argc, char** argv) {
    const int depth = argc > 1 ? std::atoi(argv[1]) : 6;
    if (depth < 1 || depth > 8) return 2;
    unsigned long long sequences = 0, checked = 0, exits = 0;
    int seq[8];
    for (int len = 1; len <= depth; ++len) {
        unsigned long long total = 1;
        for (int k = 0; k < len; ++k) total *= N_EVENTS;
        for (unsigned long long code = 0; code < total; ++code) {
            unsigned long long c = code;
            for (int k = 0; k < len; ++k) {
                seq[k] = (int)(c % N_EVENTS);
                c /= N_EVENTS;
            }
            World w;
            ++sequences;
            for (int k = 0; k < len; ++k) {
                const bool was_clean = w.clean_run;
                const bool mixed = w.mixed;
                const Verdict v = apply(w, (Event)seq[k]);
                if (seq[k] != RUN_AHEAD) continue;
                ++checked;
                const bool unsound = v.rigid_exit && mixed;
                const bool dead = was_clean && !mixed && !v.rigid_exit;
                if (v.rigid_exit) ++exits;
                if (unsound || dead) {
                    std::printf("%s after", unsound ? "a rigid exit over mixed velocities" : "no rigid exit over uniform velocities");
                    for (int j = 0; j <= k; ++j) std::printf(" [%s]", NAMES[seq[j]]);
                    std::printf("\n");
                    return 1;
                }
                w.clean_run = false;  // (the record is taken)
            }
        }
    }
    std::printf("ok %llu %llu %llu\n", sequences, checked, exits);
    return 0;
}
