// sphx_handoff.hpp — what one launch of the host step path promises a later one (sphx_ctx::handoff, sphx_ctx::pending,
// sphx_ctx::velmarks): value types with one producer side, one taking call per consumer and one reset each.  Plain C++
// (no HIP include, no HIP call): tests/handoff_driver.cpp compiles it with the sanitizers and compares it with the loose context
// members it replaced; tests/rigid_record_driver.cpp does the same for VelMarks against a model of the velocity array.
#pragma once
#include <cstdint>
#include <cstring>

namespace sphx {

// What the latest neighbour build left for the divergence loop behind it.
//   None         nothing: the loop's first iteration runs its warm start (if any) and its compute_density_change itself
//   WarmApplied  the build applied the loop's warm start (k_neighbor_build<3>)
//   FirstErrors  the build did the first compute_density_change (k_neighbor_build<2>).  has_flags: it wrote the zero-skip flags too,
//                the scene-wide mark under reduction sequence number mark_tag; warm_taken (only with flags): and stored the sums 0 + k
// update_neighborhood assigns a whole value per build of at least one particle; a taking call that finds what it asks for leaves None.
struct BuildHandoff {
    enum Kind : uint8_t { None, WarmApplied, FirstErrors };
    Kind kind = None;
    bool has_flags = false, warm_taken = false;
    uint32_t mark_tag = 0;
    struct Taken {
        bool fused, flags_usable, warm_taken;
    };
    static BuildHandoff warm_applied() { return BuildHandoff{WarmApplied, false, false, 0u}; }
    static BuildHandoff first_errors(bool flags, uint32_t tag, bool taken) { return BuildHandoff{FirstErrors, flags, flags && taken, tag}; }
    void clear() { *this = BuildHandoff{}; }
    bool first_errors_pending() const { return kind == FirstErrors; }
    // The warm start in front of a divergence loop: true = the build has applied it, nothing is to be launched.
    bool take_warm() {
        const bool applied = kind == WarmApplied;
        if (applied) clear();
        return applied;
    }
    // Asked once per solver iteration, with the reduction sequence number it publishes under.  fused: its compute_density_change is
    // done; flags_usable: and the flags carry this iteration's mark (a mark under another number says nothing about this one);
    // warm_taken: and its warm-start sums are stored.  Only a loop's first divergence iteration takes them; behind any other they stay.
    Taken take_first_errors(bool first_divergence, uint32_t rseq) {
        if (kind != FirstErrors || !first_divergence) return Taken{false, false, false};
        const bool usable = has_flags && mark_tag == rseq;
        const Taken t{true, usable, usable && warm_taken};
        clear();
        return t;
    }
};

// The cell count in gdyn.hist / key of a neighbour build that has not come yet, and who made it:
//   Nobody      the histogram is all-zero, as between any two builds
//   Correction  a single context's density correction (CountArgs), for its n particles: the step's own build starts from it
//   Pack        tile_pack_impl or sphx_tile_count_kept, for the n particles the tile keeps: the re-grid counts the arrivals only
//   Classifier  a tile's classifying density correction (TileClassArgs), from ADVECTED positions and without what the tile retires:
//               good for nothing but the packing pass that takes it over (then it is Pack's)
// No HIP call here: a drop returns whether its caller (drop_fused_count, drop_class_count) has to wipe the histogram.
// Two things the loose flags this replaces could say apart:
//  - "the classifier's count" without "a pack may take it over": a classifying sphx_sub_iteration, then sphx_tile_configure_rect,
//    sphx_tile_apply_n, a refused sphx_tile_upload or a sphx_tile_count_kept that returns early (directory about to change).  None
//    of them needs the histogram, so the count stays for the next drop_class_count, but its classification is stale: `takeable_`.
//  - "the classifier's count" without any pending count: a classifying sphx_sub_iteration, then sphx_upload / sphx_state_load
//    (clear_histograms), sphx_append / sphx_remove (drop_fused_count) or a new directory.  Nothing is left to wipe or take over and
//    every consumer was told what Nobody tells it (flush_pending_advect selects no device for a drop that issues nothing): folded.
//    (The classification's particle count and the count's own were set by the same iteration: one n.)
class PendingCount {
  public:
    enum class Maker : uint8_t { Nobody, Correction, Pack, Classifier };
    PendingCount() = default;
    // ---- producers: the count of the first n particles is on the stream (classifier: from the positions advected by dt)
    void made_by_correction(uint32_t n) { *this = PendingCount(Maker::Correction, n); }
    void made_by_pack(uint32_t n) { *this = PendingCount(Maker::Pack, n); }
    void made_by_classifier(uint32_t n, float dt) { *this = PendingCount(Maker::Classifier, n, true, bits(dt)); }
    // ---- queries
    bool live() const { return maker_ != Maker::Nobody; }
    bool from_classifier() const { return maker_ == Maker::Classifier; }
    bool is_for(uint32_t n) const { return live() && n_ == n; }           // the count of exactly these n particles
    bool is_for_first_of(uint32_t n) const { return live() && n_ <= n; }  // ... of the first n() of them
    uint32_t n() const { return n_; }
    // tile_pack_impl, for n particles about to be advected by a dt of the same bits: the classifier's count becomes the pack's
    bool take_over_class(uint32_t n, float dt) {
        const bool mine = from_classifier() && takeable_ && n_ == n && dt_bits_ == bits(dt);
        if (mine) made_by_pack(n);
        return mine;
    }
    // an entry point that changes what the classification was made for without needing the histogram
    void bar_take_over() { takeable_ = false; }
    // ---- drops: true = the histogram holds a count nobody will consume, the caller wipes it
    bool drop() {
        const bool wipe = live();
        forget();
        return wipe;
    }
    bool drop_if_from_classifier() { return from_classifier() && drop(); }
    // a build starts from the count (its k_scatter counts the histogram back down), or the histogram is gone or wiped whole
    void forget() { *this = PendingCount(); }

  private:
    PendingCount(Maker m, uint32_t n, bool takeable = false, uint32_t dt_bits = 0) : maker_(m), takeable_(takeable), n_(n), dt_bits_(dt_bits) {}
    static uint32_t bits(float f) {
        uint32_t u;
        std::memcpy(&u, &f, 4);
        return u;
    }
    Maker maker_ = Maker::Nobody;
    bool takeable_ = false;
    uint32_t n_ = 0, dt_bits_ = 0;
};

// Rigid motion: the fluid gather of a step's build (k_rank_gather) has compared every velocity it moved with vel_in[0]
// and left, under the sequence number `tag`, a mark in MarkStripe::vmix_mark wherever one differed.  While this record is valid those
// marks describe vel[]: nothing queued since can have written a velocity, except thin corrections on their marked path — which the
// host cannot know of when it queues them; the record keeps the reduction sequence number the (one) thin correction published under,
// and the consumer reads that iteration's knz_mark words beside the gather's.
//   made        build_grid, the fluid build inside a single context's step
//   thin        launch_correct queued a k_correct_thin behind the gather (a second one voids: one knz tag travels)
//   wrote       anything else that can write a velocity: k_neighbor_build<3>, a warm start, a correction in any other form, the
//               prediction, an upload, an edit, sphx_state_load, lists_went_stale, a failed call
//   take        the run-ahead non-pressure launch, once; leaves the record void whatever it finds
struct VelMarks {
    bool valid = false, thin_seen = false;
    uint32_t tag = 0, knz_tag = 0;
    struct Taken {
        bool usable, check_knz;
        uint32_t tag, knz_tag;
    };
    void made(uint32_t gather_tag) { *this = VelMarks{true, false, gather_tag, 0u}; }
    void thin(uint32_t rseq) {
        if (!valid) return;
        if (thin_seen) return wrote();
        thin_seen = true;
        knz_tag = rseq;
    }
    void wrote() { *this = VelMarks{}; }
    Taken take() {
        const Taken t{valid, valid && thin_seen, tag, knz_tag};
        wrote();
        return t;
    }
};

// Rigid motion, the acceleration array: the latest non-pressure launch was the rigid form under the gather's sequence
// number `tag`.  Its workgroup 0 has stored `tag` in VerdictLine::accel_uniform iff it found no mark — then accel[] was NOT written and
// stands for K.a, and every fluid velocity carried the bits of vel[0] when the pass ran; with a mark it stored ~tag and filled accel[].
// Two facts with two lifetimes:
//   owed     under the verdict accel[] is unwritten.  Ends when somebody writes the array: a non-pressure pass in any other form
//            (filled), the fill k_accel_materialize(tag) that read() and take() ask for in front of whoever reads the array — or when
//            the array itself is gone (filled: alloc_particles).
//   uniform  under the verdict every fluid velocity still equals vel[0]: nothing queued since the pass can have written one.  Ends
//            with everything that voids VelMarks, with broken() and rigid_forget() (velocities_written), and with the first consumer.
// made     enqueue_nonpressure's rigid branch
// read     somebody copies accel[] and leaves the velocities alone (sphx_debug_download_accel, a state blob with the WCSPH section)
// take     the first consumer of accel[], a velocity prediction.  substitute: it is the rigid form of the density producer, which reads
//          K.a from its arguments where the device word equals `tag` (Taken::k_a) and writes nothing to accel[] — an array still owed
//          stays owed to a later reader; any other consumer reads the array, behind the fill if it is owed (Taken::fill).
struct AccelUniform {
    bool owed = false, uniform = false;
    uint32_t tag = 0;
    struct Taken {
        bool fill, k_a;
        uint32_t tag;
    };
    void made(uint32_t gather_tag) { *this = AccelUniform{true, true, gather_tag}; }
    void velocities_written() { uniform = false; }
    void filled() { *this = AccelUniform{}; }
    Taken read() {
        const Taken t{owed, false, tag};
        owed = false;
        return t;
    }
    Taken take(bool substitute) {
        const bool k_a = substitute && uniform;
        const Taken t{owed && !k_a, k_a, tag};
        if (t.fill) owed = false;
        uniform = false;
        return t;
    }
};

}  // namespace sphx
