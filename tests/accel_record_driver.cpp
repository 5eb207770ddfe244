// Stand-alone driver for the acceleration record of the host step path (sphx::AccelUniform, yasph2d_amd/csrc/sphx_handoff.hpp): plain
// C++, compiled by tests/test_accel_record_host.py with the address and undefined-behaviour sanitizers (any report aborts).
//   accel_record_driver [depth]      (depth: longest sequence, default 6)
// The MODEL is the device, reduced to what the record speaks about:
//   accel[]      `array_current` — the array holds what the latest non-pressure pass computed; `latest_is_ka` — what that pass computed
//                is K.a for every particle (it was the rigid form and found no mark)
//   vel[]        `mixed` — some velocity's bits differ from vel[0]'s; `written_since` — a velocity was written since the latest pass
//   the word     VerdictLine::accel_uniform as k_nonpressure_rigid's workgroup 0 stores it
// Next to it stands the host code of sphx_launch.inc written with the record (enqueue_nonpressure, sphx_step_begin_law's adoption,
// take_accel / read_accel with k_accel_materialize, launch_compute_error's choice of form).  Both are driven through every sequence of
// the events below up to the given length; at every reader of accel[] the driver checks
//   soundness 1: a consumer reads K.a from its arguments only when the model's array stands for K.a over uniform velocities that
//                nothing has written since the pass;
//   soundness 2: nobody reads an accel[] that does not hold the latest pass's result (a pass must have run: a download in front of
//                the first pass reads what the allocation left, with or without the record);
//   liveness:    a rigid pass without a mark, debug downloads at most, then the adopting step with the take-over producer: K.a comes
//                from the arguments.
// Prints "ok <sequences> <reads checked> <reads of K.a from the arguments> <fills that wrote>" and returns 0, or the first offending
// sequence and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "sphx_handoff.hpp"

using namespace sphx;

enum Event {
    RIGID_AHEAD,         // enqueue_run_ahead -> enqueue_nonpressure's rigid branch; the device finds a mark iff the velocities are mixed
    FULL_AHEAD,          // enqueue_run_ahead, the pass in today's form
    BEGIN_TAKEOVER,      // sphx_step_begin_law: adopts the pass or runs it again in full; the fused producer in its take-over form
    BEGIN_FUSED,         // ... the fused producer in another form (no flags, no take-over): it reads the array
    BEGIN_PREDICT,       // ... a density warm start or SPHX_FUSE_PREDICT=0: launch_predict
    WARMSTART,           // launch_warmstart / a correction: velocities written behind the pass
    UPLOAD_MIXED,        // sphx_upload with other velocities: the pass that ran ahead is not adopted
    UPLOAD_UNIFORM,      // sphx_upload with one velocity
    EDIT,                // sphx_append / sphx_remove
    STATE_LOAD,          // sphx_state_load (a DFSPH blob: no accelerations in it)
    FAILED_CALL,         // sphx_ctx::fail on a refused argument: nothing on the device changes, the pass stays adoptable
    BROKEN,              // sphx_step_finish's broken(): the arrays are mid-step
    DEBUG_DOWNLOAD,      // sphx_debug_download_accel
    N_EVENTS
};
static const char* const NAMES[N_EVENTS] = {"rigid pass",     "full pass", "begin take-over", "begin fused", "begin predict", "warm start", "upload mixed",
                                            "upload uniform", "edit",      "state load",      "failed call", "broken",        "download"};

struct World {
    // the device
    bool array_current = false, latest_is_ka = false, any_pass = false;
    bool mixed = false, written_since = false;
    uint32_t word = 0;
    // the host
    uint32_t gather_seq = 0;
    bool ahead = false;  // sphx_ctx::ahead.queued && valid
    AccelUniform rec;
    // liveness bookkeeping: an unmarked rigid pass, nothing but downloads since
    bool clean = false;
};

struct Tally {
    unsigned long long reads = 0, from_args = 0, fills = 0;
};

static const char* full_pass(World& w) {
    w.array_current = true;
    w.latest_is_ka = false;
    w.any_pass = true;
    w.written_since = false;
    w.rec.filled();
    w.clean = false;
    return nullptr;
}
// k_accel_materialize under t.tag
static const char* fill(World& w, const AccelUniform::Taken& t, Tally& n) {
    if (!t.fill || w.word != t.tag) return nullptr;
    if (!w.latest_is_ka) return "a fill of K.a over a pass that computed something else";
    w.array_current = true;
    ++n.fills;
    return nullptr;
}
static const char* read_array(const World& w, Tally& n) {
    ++n.reads;
    return w.any_pass && !w.array_current ? "a read of an accel[] that nobody wrote" : nullptr;
}
static const char* begin(World& w, Event e, Tally& n, bool& from_args) {
    const bool adopted = w.ahead;
    w.ahead = false;
    if (!adopted) full_pass(w);  // (enqueue_nonpressure without marks: today's form)
    const AccelUniform::Taken t = w.rec.take(e == BEGIN_TAKEOVER);
    if (const char* bad = fill(w, t, n)) return bad;
    const char* bad = nullptr;
    if (t.k_a && w.word == t.tag) {  // k_compute_error_rigid under the verdict
        ++n.reads;
        ++n.from_args;
        from_args = true;
        if (!w.latest_is_ka || w.mixed || w.written_since) bad = "K.a from the arguments over an array or velocities that do not stand for it";
    } else {
        bad = read_array(w, n);
    }
    w.written_since = true;  // the prediction
    if (!w.latest_is_ka) w.mixed = true;
    return bad;
}

static const char* apply(World& w, Event e, Tally& n, bool& from_args) {
    switch (e) {
    case RIGID_AHEAD: {
        if (++w.gather_seq == 0) w.gather_seq = 1;
        const uint32_t tag = w.gather_seq;
        const bool marked = w.mixed;
        w.word = marked ? ~tag : tag;
        w.array_current = marked;
        w.latest_is_ka = !marked;
        w.any_pass = true;
        w.written_since = false;
        w.rec.made(tag);
        w.ahead = true;
        w.clean = !marked;
        return nullptr;
    }
    case FULL_AHEAD:
        full_pass(w);
        w.ahead = true;
        return nullptr;
    case BEGIN_TAKEOVER:
    case BEGIN_FUSED:
    case BEGIN_PREDICT: {
        const char* bad = begin(w, e, n, from_args);
        w.clean = false;
        return bad;
    }
    case WARMSTART:
        w.rec.velocities_written();
        w.mixed = w.written_since = true;
        w.clean = false;
        return nullptr;
    case UPLOAD_MIXED:
    case UPLOAD_UNIFORM:
    case EDIT:
    case STATE_LOAD:
        w.ahead = false;
        w.rec.velocities_written();  // rigid_forget / lists_went_stale
        w.mixed = e != UPLOAD_UNIFORM;
        w.written_since = true;
        w.clean = false;
        return nullptr;
    case FAILED_CALL:
        w.rec.velocities_written();  // fail() -> rigid_forget
        w.clean = false;
        return nullptr;
    case BROKEN:
        w.ahead = false;
        w.rec.velocities_written();
        w.mixed = w.written_since = true;
        w.clean = false;
        return nullptr;
    case DEBUG_DOWNLOAD: {
        const AccelUniform::Taken t = w.rec.read();
        if (const char* bad = fill(w, t, n)) return bad;
        return read_array(w, n);
    }
    default:
        return nullptr;
    }
}

int main(int argc, char** argv) {
    const int depth = argc > 1 ? std::atoi(argv[1]) : 6;
    if (depth < 1 || depth > 7) return 2;
    unsigned long long sequences = 0;
    Tally n;
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
                const bool was_clean = w.clean;
                bool from_args = false;
                const char* bad = apply(w, (Event)seq[k], n, from_args);
                if (!bad && seq[k] == BEGIN_TAKEOVER && was_clean && !from_args) bad = "no K.a from the arguments behind an unmarked rigid pass";
                if (bad) {
                    std::printf("%s after", bad);
                    for (int j = 0; j <= k; ++j) std::printf(" [%s]", NAMES[seq[j]]);
                    std::printf("\n");
                    return 1;
                }
            }
        }
    }
    std::printf("ok %llu %llu %llu %llu\n", sequences, n.reads, n.from_args, n.fills);
    return 0;
}
