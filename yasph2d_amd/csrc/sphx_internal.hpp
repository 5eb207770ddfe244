// sphx_internal.hpp — shared declarations of libsphx (device context, constants, launch/profiling helpers).
#pragma once
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/sphx.h"
#include "sphx_handoff.hpp"

namespace sphx {

constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr uint32_t MAX_NEIGHBORS = 64;  // neighborhood_search.rs:322
constexpr uint32_t BLOCK_SHIFT = 6;     // directory blocks are 64x64 cells
constexpr uint32_t BLOCK_CELLS = 4096;  // cells per block = low 12 Morton bits
constexpr uint32_t SCAN_TILE = 4096;    // elements per workgroup of the two-launch scan (256 threads x 16)
#ifndef SPHX_SCAN_ITEMS
#define SPHX_SCAN_ITEMS 16
#endif
constexpr uint32_t SCAN1_ITEMS = SPHX_SCAN_ITEMS;        // one-launch (look-back) scan: table entries per thread (a multiple of 4)
constexpr uint32_t SCAN1_TILE = 256 * SCAN1_ITEMS;       // ... per workgroup
#ifndef SPHX_STAGE_ROWS
#define SPHX_STAGE_ROWS 12
#endif
#ifndef SPHX_WIN_HALO
#define SPHX_WIN_HALO 116  // (round 4: 116 instead of 128 — with the window of velocities the build then fits 20 KiB of LDS, eight workgroups per CU)
#endif
constexpr uint32_t STAGE_ROWS = SPHX_STAGE_ROWS;     // neighbour rows staged in LDS per wave before the coalesced row store
constexpr uint32_t WIN_HALO = SPHX_WIN_HALO;      // neighbour build: positions of [block_first - 128, block_last + 128] are staged in LDS (256: same speed at 6 instead of 7 workgroups per CU in the form that also stages velocities)
#ifndef SPHX_LIST_HALO
#define SPHX_LIST_HALO 116  // (= SPHX_WIN_HALO: the build's window of positions is the traversals' window)
#endif
// Neighbour lists are WORKGROUP-LOCAL: the traversal kernels stage the records of the sorted slots
// [block_first - LIST_HALO, block_last + LIST_HALO] in LDS with coalesced loads; a list entry < LIST_WIN is a slot of that window,
// an entry >= LIST_WIN indexes the workgroup's table of out-of-window neighbours (REMOTE_CAP global record indices, staged behind
// the window).  Every neighbour record is then read from LDS.
constexpr uint32_t LIST_HALO = SPHX_LIST_HALO;
constexpr uint32_t LIST_WIN = 256 + 2 * LIST_HALO;
constexpr uint32_t REMOTE_CAP = 512;
// a narrow list entry = a slot of the staging area (window + out-of-window table = 1024 slots): ten bits, three to the 32-bit word
// a lane owns in one sub-row of its wavefront's slice, each stored as the slot's byte offset in a 4-byte array (pack3, sphx_kernels.hip)
constexpr uint32_t ENTRY_BITS = 10, ENTRY_MASK = (1u << ENTRY_BITS) - 1u;
constexpr uint32_t WAVE_REMOTE = REMOTE_CAP / 4;  // every wavefront of a workgroup owns a quarter of the table (its format is decided per wavefront)
constexpr uint32_t STRIPES = 32;        // same-address atomics serialise in L2: counters are striped over 32 cache lines

// internal device flag bits (DevScalars::flags)
constexpr uint32_t DIR_FRINGE = 0x80000000u;  // directory entry flag: a covered block on the fringe of the fluid (offsets stay < 2^31)
constexpr uint32_t DIR_STATIC = 1u;  // dynamic directory only: the boundary's directory covers this block too (offsets are multiples of 4096)
constexpr uint32_t DIR_FLAGS = DIR_FRINGE | DIR_STATIC;
enum : uint32_t { DF_OUT_OF_DOMAIN = 1u, DF_HALO_CAP = 2u, DF_NB_CAP = 4u, DF_NB_PANIC = 8u, DF_NEAR_EDGE = 16u, DF_STRAY = 32u, DF_SCAN_STALL = 64u, DF_NONFINITE = 128u, DF_DENSE_CELL = 256u };
constexpr uint32_t RANK_LOOP_MAX = 4096;  // k_rank_gather: largest cell whose particles are ranked by previous index (quadratic in the occupancy)
constexpr uint32_t LOOP_HIST = 512;  // residual sums of the latest solver loop kept in the mailbox (ring; the reference caps a loop at 200 / 400 (+1) iterations)

// Constants every kernel needs; passed by value (kernarg).  Derived exactly like the reference's constructors.
constexpr uint32_t MAX_TILE_PEERS = 8;  // a rectangle has at most 8 neighbours (4 edges + 4 corners) in a regular tiling
struct TileRect {
    uint32_t x0, x1, y0, y1;  // cells, half-open
};

struct Consts {
    float h;         // smoothing length = search radius = cell size
    float radius_sq; // grid.radius * grid.radius (neighborhood_search.rs:331)
    float cell_inv;  // 1 / cell_size (neighborhood_search.rs:475)
    float gmin_x, gmin_y;
    float w_hinv, w_norm, w_ngrad;   // WendlandQuinticC2::new (wendland_quintic_c2.rs:24-30)
    float p6_hsq, p6_norm, p6_ngrad; // Poly6::new (poly6.rs:16-23)
    float sp_h, sp_norm, sp_ngrad;   // Spiky::new (spiky.rs:16-23)
    float mass, rho0, xsph_eps;
    float ax, ay;    // non_pressure_accelleration = gravity*m/m (dfsph.rs:442-444)
    float gx, gy;    // gravity itself (wscsph.rs:83)
    float wc_stiffness, wc_boundary_force;  // WCSPHSolver::set_compressibility(.., 0.01, 1.0), boundary_force_factor (wscsph.rs:31-49)
    // spatial tile owned by this context (multi-GPU): the cell rectangle [x0,x1) x [y0,y1); reductions only count owned
    // particles.  Single-GPU default: the whole domain.
    TileRect tile;
    // a workgroup with at most remote_cap out-of-window neighbour entries stores workgroup-local 10-bit lists (<= REMOTE_CAP;
    // 0 forces 32-bit global lists)
    uint32_t remote_cap;
    // 1: the walks may use their FAST forms (sphx_kernels.hip, sqrt_dist): the lists belong to the positions (raised by the neighbour
    // build, dropped by an upload) and fl(r * w_hinv) <= 1 for every r a list can hold (r <= h: checked by the host for this h), i.e.
    // the min(q, 1) of WendlandQuinticC2::evaluate / gradient (wendland_quintic_c2.rs:35,43) is the identity and the sqrt's argument
    // is far from the ends of the exponent range
    uint32_t q_noclamp;
    uint32_t nt_cold;  // outputs that nobody reads before the next step (density, alpha, warm-start sums, ids) are stored with the nontemporal hint
    uint32_t xcd_shift;  // log2 of the XCD chunk length in blocks (xcd_bid; 0: contiguous eighths)
    uint32_t rev;  // this launch sweeps the particle blocks from the top down (xcd_bid; alternates from launch to launch, sphx_ctx::alternate_sweep)
};

// The viscosity model (sphx_params.viscosity_model; PhysicalViscosityModel, physical.rs, with the Viscosity kernel's Laplacian,
// viscosity.rs:19-47).  Kept out of Consts on purpose: Consts travels by value in the middle of every kernel's argument list, and
// three more words there would move the kernel-argument offsets of every kernel.  The model is a compile-time choice of the two
// kernels that evaluate it (k_nonpressure, k_wcsph_accel); only their physical instantiations take this struct as a trailing
// argument, the XSPH ones an empty ViscArg that occupies no kernel-argument space, so their code is the code from before.
struct ViscConsts {
    uint32_t visc_model;  // SPHX_VISCOSITY_* (host dispatch only)
    float mu;             // PhysicalViscosityModel::fluid_viscosity
    float vis_nlap;       // Viscosity::normalizer_laplacian = 360 / ((29 pi) h^5), viscosity.rs:24
};
template <int VM>
struct ViscArg {};
template <>
struct ViscArg<SPHX_VISCOSITY_PHYSICAL> : ViscConsts {};

// wave-sliced neighbour lists (one 16 KiB slice per 64 particles); counts[i] = count_dynamic | count_total << 7 = NeighborRange
// (neighborhood_search.rs:269-273) in 16 bits; wave[i >> 6] = entries of the wavefront's quarter of the out-of-window table
// remote[(i >> 8) * REMOTE_CAP + ((i >> 6) & 3) * WAVE_REMOTE ..] | wide << 31 (the list format is decided per wavefront)
struct NbView {
    const uint32_t* list;
    const uint16_t* counts;
    const uint32_t* wave;
    const uint32_t* remote;
    // round 4: the upper 64 lines of a wavefront's out-of-window table are only fetched when the wavefront uses more than 64 (bit 14 of
    // its particles' count words says so: known from a load every walk makes first anyway, and by the time the branch waits for it
    // everything else the walk needs has been requested).  4 bytes per particle and walk less: the traversals -1...-4 % at 16 M, nothing
    // lost at 1 M (same-box A/B, profiles/r04_experiments/lazy_table_ab.txt; round 3 had tried the per-wavefront word as the condition —
    // a scalar load of its own — and lost 3 % at 1 M).  SPHX_LAZY_TABLE=0 turns it off.
    uint32_t lazy_hi;
    // round 4: list words and table lines are read exactly once per walk; a context whose lists do not fit the caches anyway (>= 4 M
    // particles) reads them with the nontemporal hint (-1 % at 16 M; at 1 M, where the lists of one walk are still in the Infinity
    // Cache for the next, the hint costs 1-5 %: profiles/r04_experiments/scan_touched_tiles.txt).  SPHX_STREAM_LISTS=0/1 overrides.
    uint32_t stream;
};
constexpr uint32_t COUNT_MANY_LINES = 1u << 14;  // count word: the wavefront's table holds more than 64 lines
// positions + velocities of the [N|B] arrays as one read view (sphx_kernels.hip: ldpv)
struct PVr {
    const float2* pos;
    const float2* vel;
};

// Two-level Morton cell grid.  dir[] is a small host-built 2D directory over the 64x64-cell blocks of the
// covered rectangle: dir[(by-by0)*nbx + (bx-bx0)] = offset of the block's 4096 fine entries, or EMPTY.  Blocks are numbered in
// ascending Morton order of (bx,by) and cells inside a block by the low 12 bits of their Morton code, so the fine table is in
// GLOBAL Morton order: fine[i] = {first, one-past-last} sorted particle of cell i (exclusive prefix sum of the per-cell
// histogram).  The table length is known on the host.
struct GridView {
    const uint32_t* dir;
    const uint2* fine;  // {first sorted particle of the cell, one past its last}
    uint32_t bx0, by0, nbx, nby;
};
// The same grid as the neighbour build reads it (round 4): a second directory `dirn` in which NO entry is special —
//   * a block the directory does not cover points at the NULL BLOCK, 4096 all-zero entries behind the cell table ({0, 0}: an empty
//     range), so the nine look-ups of a 3x3 box need no "is it covered" select, neither on the slot nor on the range;
//   * block coordinates outside the directory's rectangle are CLAMPED into it (nbx1 = nbx - 1, nby1 = nby - 1) instead of tested:
//     what such a look-up finds are the cells of some other block with the same local coordinates — 60 or more cells away, every
//     candidate fails the distance test, and a cell never aliases one of the box's own (their local coordinates differ);
//   * bit 0 (DIRN_FLAG) of an entry — dynamic grid: the boundary's directory covers this block or one of its eight neighbours
//     (only then can a particle of the block have static neighbours; null entries carry it always); static grid: the block is covered.
// An empty directory is presented as one null entry.
struct NbGrid {
    const uint32_t* dirn;
    const uint2* fine;
    uint32_t bx0, by0, nbx, nbx1, nby1;
};
constexpr uint32_t DIRN_FLAG = 1u;

struct alignas(128) Stripe {
    unsigned long long nb_entries;  // partial sum of count_total over ALL builds so far (stats only; the host takes differences)
    unsigned long long owned;       // partial count of owned particles over ALL tile re-grids so far (host takes differences)
    unsigned long long rem_entries; // partial sum of out-of-window list entries over ALL builds so far (stats only)
    // Reductions without a tail: a workgroup adds its share with fire-and-forget integer atomics and is gone; the
    // NEXT kernel on the stream reads the 32 stripes.  res_hi/res_lo: residual sums in 2^-24 fixed point, cumulative over ALL
    // iterations so far (never reset: readers take differences); vmax[]: max |v + a dt|^2 bits, a ring of 4 (the reader of slot v
    // clears slot v + 2).
    unsigned long long res_hi, res_lo;
    uint32_t ticket;                // first-level arrival counter of the last-block reduction (two-pass scan only)
    uint32_t pad0;
    // zero-correction skip (k_correct), cumulative, collected only with SPHX_ZERO_SKIP_COUNT=1: workgroups that skipped
    // their walk / that a flag of their window stopped / that a flag behind an out-of-window table line stopped
    unsigned long long zs_skipped, zs_window, zs_remote;
    unsigned long long zs_quiet;    // ... and, of the skipped ones, those that left through the quiet-scene exit (decide-first form)
    // rigid form of the density producer (k_compute_error_rigid), the same switch: workgroups that left through the fluid-only exit /
    // that walked with K.a from the arguments; launches whose workgroup 0 found no verdict (sphx_debug_rigid_predict_counts)
    uint32_t rp_exit, rp_walk, rp_noverdict;
    uint32_t pad[9];
};
static_assert(sizeof(Stripe) == 128, "one stripe, one cache line");
// The max-velocity ring lives on cache lines of its own: the first density iteration READS it (velocity prediction folded into
// compute_density_error) while workgroups of the same launch that have finished ADD their residual to Stripe — with both on one
// line every one of those atomics sent the readers of that line back to the fabric (19.5 -> 31.7 us per launch at 1M particles
// once the residuals are non-zero, profiles/r03_experiments/predict_fusion.txt).
struct alignas(128) VmaxStripe {
    uint32_t vmax[4];
    uint32_t pad[28];
};
// Scene-wide "some k is not +-0" mark (knz_store): the reduction sequence number (ResArgs::rseq) of the latest iteration in which a
// wavefront of a workgroup with this stripe number stored a k other than +-0.  Never reset: a reader compares with its own number.
// On lines of its own, for the reason VmaxStripe is: a first form kept the word in Stripe's padding, where the plain stores of a
// disturbed scene's wavefronts met the residual atomics of the same launch — compute_density_error 198.9 -> 253.6 us and
// compute_density_change 135.9 -> 164.5 us at 16 M, 2500 steps in (profiles/quiet_scene/ab_16M_1M.txt).
// vmix_mark (rigid motion): the sequence number of the latest fluid gather in which a wavefront of a workgroup with this
// stripe number moved a velocity whose bits differ from vel_in[0]'s (or found vel_in[0] not finite).  The same scheme: a tag unique to
// the launch, no reset, an accidental match reads as "mixed".  It shares knz_mark's line: plain stores only, by a kernel (the gather)
// that runs while nobody reads or writes the other word.
struct alignas(128) MarkStripe {
    uint32_t knz_mark;
    uint32_t vmix_mark;
    uint32_t pad[30];
};
static_assert(sizeof(MarkStripe) == 128, "one stripe, one cache line");
// Quiet take-over of the density loop: the cell count compute_density_error makes ahead of its correction is
// speculative — right iff the correction turns out to be the identity — and so are the DF_* flags that count raises.  They wait
// here, on a line no residual, mark or sticky flag shares, until the thin correction merges them into DevScalars::flags (quiet) or
// drops them (marked: its recount raises the real ones).  moved: particles whose cell a recount changed (SPHX_ZERO_SKIP_COUNT=1).
struct alignas(128) SpecLine {
    uint32_t flags;
    uint32_t pad0;
    unsigned long long moved;
    uint32_t pad[28];
};
// The verdict of the latest rigid non-pressure launch (k_nonpressure_rigid's workgroup 0, a plain store): the gather's tag when it found
// no mark and left accel[] unwritten (it stands for K.a), ~tag when it filled the array.  Never reset: a reader compares with the tag
// the host handed it (sphx::AccelUniform).  On a line of its own — every workgroup of the density producer's rigid form reads it
// while finished workgroups of the same launch add their residuals to Stripe (knz_mark's lesson).
struct alignas(128) VerdictLine {
    uint32_t accel_uniform;
    uint32_t pad[31];
};
struct DevScalars {
    uint32_t flags;        // DF_*
    uint32_t ticket;       // second-level arrival counter (one arrival per stripe); reset by the last arriver
    uint32_t sort_total;   // number of particles that received a cell in the latest histogram scan (tile mode: new local count)
    float dt;              // time step the device derived from vmax with the host's timer law (sphx_step_begin_law)
    uint32_t loop_done;    // solver loop run by the device (LoopArgs): 0 while it iterates, else the iteration that met the residual test
    uint32_t pad0;
    unsigned long long snap_hi[2], snap_lo[2];  // cumulative residual sums after the iteration with reduction sequence number r at [r & 1]
    uint32_t rigid_exits, rigid_marked;  // rigid non-pressure launches that found no mark / a mark (one add per launch; sphx_debug_rigid_counts)
    uint32_t pad[16];
    Stripe stripe[STRIPES];
    VmaxStripe vstripe[STRIPES];
    MarkStripe mstripe[STRIPES];
    SpecLine spec;
    VerdictLine verdict;
};

// Pinned, host-coherent memory the device publishes step scalars into (no D2H copy, no stream sync on the fast path).
struct Mailbox {
    volatile uint32_t seq;  // written last (system scope); the host waits for the value it passed to the kernel
    uint32_t flags;
    uint32_t vmax_sq_bits;  // max |v + a*dt|^2 as float bits
    // quiet-scene hint (k_correct): a correction launched with flags writes its own `seq` here when no stripe carries its
    // iteration's mark (every k of the scene is +-0), else 0; written before seq, like err_sum.  Other corrections leave it alone.
    uint32_t quiet_seq;
    double err_sum;         // residual sum of the last compute_error launch
    unsigned long long nb_entries;
    unsigned long long owned_cum;
    unsigned long long rem_entries;
    uint32_t sort_total;
    uint32_t dt_bits;       // sphx_step_begin_law: the device's dt (float bits) ...
    unsigned long long dt_ns;  // ... and the Duration it came from
    // solver loop terminated by the device (LoopArgs): written by the iteration that met the residual test, BEFORE its seq
    volatile uint32_t loop_gen_done;  // generation number of the loop that has finished
    uint32_t loop_iters;              // ... after this many iterations
    double loop_hist[LOOP_HIST];      // residual sum of iteration k of the running loop at [k % LOOP_HIST] (the host re-derives every decision)
    uint32_t send_counts[MAX_TILE_PEERS];  // sphx_tile_send_counts: landing place of the headers' record counts (host copies, no kernel writes here)
    // rigid-motion hint: the wavefront that judges the marks for a non-pressure pass (k_nonpressure_rigid's workgroup 0,
    // k_rigid_judge) writes the gather's tag here when no stripe carries a mark, else 0.  Read behind the seq of the kernel queued
    // behind the pass (the velocity prediction publishes its maximum).
    uint32_t rigid_tag;
};

// A solver loop (dfsph.rs:195-247 / :346-402) whose termination test runs on the device: the last workgroup of compute_error
// holds the residual sum, applies dfsph.rs:221-236 / :376-391 to it and records the outcome in DevScalars::loop_done; iterations
// queued behind the terminating one return at once, and the density correction of the terminating iteration (it knows it is the
// last) does the re-grid's advection + cell count.  The host verifies every decision from loop_hist afterwards.
// Who reads a reduction: the kernel queued behind the one that produced it.  Every workgroup of the reader derives the same value
// from the stripes; its workgroup 0 publishes to the mailbox.
struct ResArgs {  // reader of the residual sum of a compute_error launch (the correction of the same iteration)
    uint32_t enabled;
    uint32_t rseq;  // reduction sequence number of this iteration (the context counts them; consecutive)
    Mailbox* mb;
    uint32_t seq;   // mailbox sequence number the residual is published under
};
struct VmaxArgs {  // reader of max |v + a dt|^2 (the velocity prediction, or k_publish_vmax)
    uint32_t enabled;
    uint32_t vslot;  // ring slot the producer used
    Mailbox* mb;
    uint32_t seq;
};
struct LoopArgs {
    uint32_t enabled;    // 0: host-driven loop (tile mode: the residual needs an all-reduce over the ranks)
    uint32_t iter;       // 1-based index of this iteration
    uint32_t fixed;      // sphx_params.fixed_*_iterations
    uint32_t max_iters;  // dfsph.rs:50 / :54
    uint32_t gen;        // generation number of this loop
    uint32_t n_total;    // particles the average runs over
    float tol;           // dfsph.rs:49 / :53
    float rho0;
    float dt;            // the step (host value; kernels given dt_dev use the device's)
};

// TimeManager::update_simulation_step (timemanager.rs:252-279) as the device applies it to its own vmax
struct TimerLaw {
    uint32_t enabled, adaptive;
    float cfl_factor, particle_diameter;
    unsigned long long min_ns, max_ns, step_ns;
};

struct Grid {
    uint32_t* dir = nullptr;   // nbx*nby entries
    uint32_t* dirn = nullptr;  // the neighbour build's form of it (NbGrid), max(nbx*nby, 1) entries
    uint32_t dir_cap = 0;
    uint2* fine = nullptr;     // cell ranges of the latest build (len() entries) + the null block (BLOCK_CELLS all-zero entries)
    uint32_t* hist = nullptr;  // all-zero between builds; receives the next build's per-cell histogram
    uint32_t* tile_empty = nullptr;  // per scan tile: held no particle at the latest build (k_scan_onepass); tile_cap entries
    uint32_t tile_cap = 0;
    uint32_t fine_cap = 0;     // entries allocated in fine and hist
    uint32_t bx0 = 0, by0 = 0, nbx = 0, nby = 0, nblk = 0;
    std::vector<uint8_t> cover;  // dynamic grid, host side: 0 uncovered / 1 interior / 2 fringe per block of the rectangle (static grid: 0 / 1)
    std::vector<uint32_t> h_dir;  // host copy of dir
    bool fine_valid = false;      // `fine` holds the cell ranges of a build made with THIS directory
    uint32_t len() const { return nblk * BLOCK_CELLS; }
    GridView view() const { return GridView{dir, fine, bx0, by0, nbx, nby}; }
    NbGrid nview() const { return nbx && nby ? NbGrid{dirn, fine, bx0, by0, nbx, nbx - 1u, nby - 1u} : NbGrid{dirn, fine, 0u, 0u, 1u, 0u, 0u}; }
};

struct ProfTotals {
    uint64_t launches = 0;
    double ms = 0, bytes = 0;
};
struct ProfPending {
    const char* name;
    double bytes;
    hipEvent_t a, b;
};

}  // namespace sphx

struct sphx_ctx {
    sphx_params P;
    sphx::Consts K;
    sphx::ViscConsts VK;  // the viscosity model's constants (set by sphx_create, next to K)
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;

    uint32_t N = 0, capN = 0;  // fluid particles
    uint32_t B = 0, capB = 0;  // boundary particles
    uint32_t cached_n = 0;     // alpha_values.len() of the reference (dfsph.rs:419)
    // sphx_append / sphx_remove (sphx_edit.inc) changed the particle set: the next sphx_step_begin runs the warm-up block even when the
    // count has come back to cached_n (the lists belong to another set).  Cleared by that warm-up and by sphx_upload.
    bool set_changed = false;
    uint64_t ids_issued = 0;   // particles uploaded or appended since the last sphx_upload: the first id sphx_append hands out
    uint32_t* edit_buf = nullptr;  // sphx_remove: survivors per workgroup, then their exclusive scan and the total; grown on demand
    uint32_t edit_cap = 0;         // ... in 4-byte words
    // sphx_tile_remove_mark (sphx_multi_edit.inc) shares the buffer: the workgroups' words of the pass in flight, whose total
    // sphx_tile_remove_fetch reads at edit_buf[edit_mark]; sphx_tile_append stages its records there
    static constexpr uint32_t MARK_NONE = 0xFFFFFFFFu, MARK_EMPTY = 0xFFFFFFFEu;  // no pass in flight / a pass over zero records
    uint32_t edit_mark = MARK_NONE;
    // particle tracking (sphx_track_*, sphx_download_by_id: sphx_track.inc).  Belongs to the context, not to the particle state.
    // A tile (sphx_tile_track_*) keeps the shared tables of its multi here: table | filter | found, no map, m == unique; its rec is
    // [max_frames][unique] {x, y, vx, vy}, then [max_frames][unique] presence words.
    struct Track {
        uint32_t m = 0, unique = 0, log2_bits = 0;  // caller ids, distinct ids, log2 of the filter's bits
        uint32_t* set_buf = nullptr;  // device: table[unique] | map[m] | filter[2^log2_bits / 32] | found[unique]
        uint32_t *table = nullptr, *map = nullptr, *filter = nullptr, *found = nullptr;  // ... the pieces of set_buf
        float* rec = nullptr;         // recording: max_frames frames of m {x, y, vx, vy}
        uint32_t recording = 0, max_frames = 0, every = 0, frames = 0, dropped = 0, steps = 0;  // steps: finished since sphx_track_record
        uint32_t* scratch = nullptr;  // window index of sphx_download_by_id + the outputs' device copies on the host-pointer paths
        size_t scratch_cap = 0;       // ... in 4-byte words
        uint32_t window_cap = 0;      // a tile (sphx_tile_track_window_*): the record capacity of the window pass in flight
    } track;
    // fluid statistics (sphx_fluid_stats, sphx_stats_*: sphx_stats.inc).  Belongs to the context, not to the particle state.
    struct Stats {
        sphx_stats_rec* scratch = nullptr;  // device: stage-1 partial records, then the records of one host-pointer call; allocated on first use
        sphx_stats_rec* rec = nullptr;      // recording: max_frames frames of 1 + n_rects records
        sphx_rect rects[SPHX_STATS_MAX_RECTS] = {};  // ... its rectangles
        uint32_t n_rects = 0, recording = 0, max_frames = 0, every = 0, frames = 0, dropped = 0, steps = 0;  // steps: finished since sphx_stats_record
        std::vector<sphx_stats_frame> info;  // ... and one entry per stored frame (host)
    } stats;
    // gauges and probes (sphx_gauge_levels, sphx_probe_*: sphx_gauge.inc).  Belongs to the context, not to the particle state.
    struct Probe {
        uint32_t* scratch = nullptr;  // device, one-shot call: gauge table | values (unless the caller's array takes them) | host path: records
        size_t scratch_cap = 0;       // ... in 4-byte words
        uint32_t* fixed = nullptr;    // recording, device: gauge table [8 n_gauges] | values [total] | points [2 m_points]
        uint32_t* rec = nullptr;      // recording, device: [max_frames][m_points] sphx_probe_rec, then [max_frames][n_gauges] sphx_gauge_rec
        uint32_t m_points = 0, n_gauges = 0, total = 0;  // total: samples of all gauges
        int kind = 0, field = 0;
        float iso = 0.0f;
        uint32_t recording = 0, max_frames = 0, every = 0, frames = 0, dropped = 0, steps = 0;  // steps: finished since sphx_probe_record
        std::vector<sphx_stats_frame> info;  // one entry per stored frame (host)
        // a tile context (sphx_tile_gauge_* / sphx_tile_probe_*; sphx_gauge_levels and sphx_probe_* refuse a tile, so scratch, fixed and
        // rec are its own here).  scratch: table | parts [8 n_gauges] | compact values; fixed: table | compact values [total] | points;
        // rec: [max_frames][m_points] sphx_probe_rec with the "answered" mark, then [max_frames][n_gauges] sphx_gauge_part.
        std::vector<sphx_gauge> gauges_host;    // recording: the caller's gauges (the interval table is rebuilt from them when the cuts move)
        std::vector<uint32_t> table_lo_count;   // recording: the host's intervals {lo, count} per gauge the device table holds
        uint32_t table_rect[4] = {0, 0, 0, 0};  // ... and the owned rectangle they were built for
        bool table_valid = false;
        uint32_t table_owned = 0;               // ... and their samples
        std::vector<uint32_t> frame_lo_count;   // recording: the intervals of every stored frame [frames][2 n_gauges]
        uint32_t shot_gauges = 0, shot_owned = 0;  // one-shot call in flight between sphx_tile_gauge_levels and _fetch
        std::vector<uint32_t> shot_lo_count;
    } probe;
    bool uploaded = false, boundary_changed = true, tails_dirty = true, in_step = false;
    bool lists_current = false;  // the neighbour lists were built from the positions the arrays hold (raised by a completed build, dropped with q_noclamp)
    unsigned long long* state_dig = nullptr;  // sphx_state_*: one digest per section (device), allocated on first use
    // sphx_tile_state_pack (sphx_multi_state.inc): digests, the seven compacted sections of the owned particles and the scan's words
    uint32_t* mstate_buf = nullptr;
    size_t mstate_cap = 0;   // ... in 4-byte words
    uint32_t mstate_n = 0;   // ... and the local count of the pass that filled it
    uint32_t fast_walk_ok = 0;  // this smoothing length allows the FAST walks (sqrt_dist); K.q_noclamp = fast_walk_ok while the lists are fresh
    // field sampling (sphx_sample_*): 2 = the cell grids and density[] belong to the current positions (a build plus densities), 1 = a
    // build without densities since, 0 = positions / boundary replaced or a step open; sample_missing says what a query is waiting for
    uint32_t sample_ready = 0;
    bool tile_density_ready = false;  // tile mode: density[] is that of the last sphx_sub_regrid* and the positions have not moved since
    const char* sample_missing = "no neighbour build yet: run a step, or sphx_update_neighborhood + sphx_update_densities";
    float* sample_buf = nullptr;  // device scratch of the host-pointer queries (points + outputs), grown on demand
    size_t sample_cap = 0;        // ... in 4-byte words
    // sphx_tile_sample_* (a tile context; sample_buf is its scratch too — sphx_sample_* refuse a tile): the query in flight between
    // the enqueue half and the fetch half, and the null grid a tile without a dynamic (or static) grid walks instead
    struct TileSample {
        uint32_t m = 0;                    // points of the queued points query (0: none queued)
        uint32_t fields = 0;               // SPHX_SAMPLE_* bits of the queued query
        uint32_t win[4] = {0, 0, 0, 0};    // lattice window [0], [1]) x [2], [3]) of the queued window query (empty: nothing to fetch)
        size_t rec_at = 0;                 // word offset of the records in sample_buf (points query)
        uint32_t* null_grid = nullptr;     // device: BLOCK_CELLS empty ranges, then two one-entry directories (flagged / unflagged)
    } tsample;
    uint32_t* contour_buf = nullptr;  // sphx_surface_contour: lattice values, workgroup offsets (+ the outputs' device copies on the host-pointer path), grown on demand
    size_t contour_cap = 0;           // ... in 4-byte words
    // sphx_query_radius / sphx_select (sphx_query.inc): workgroup offsets, prefixes and the host-pointer path's points / per-point outputs;
    // and the entries' device copies of the host-pointer paths, sized once the total is known.  Both grown on demand.
    uint32_t* query_buf = nullptr;
    size_t query_cap = 0;             // ... in 4-byte words
    uint32_t* query_ent = nullptr;
    size_t query_ent_cap = 0;         // ... in 4-byte words
    // sphx_tile_query_* / sphx_tile_select* (a tile context; query_buf, query_ent and edit_buf are its scratch too — sphx_query_radius and
    // sphx_select refuse a tile): the call in flight between the enqueue half and the fetch half.  An enqueue of either drops both.
    struct TileQuery {
        uint32_t stage = 0;  // 0: none, 1: counted (the totals are on the device), 2: sized (totals read, entries and offsets final on the stream)
        uint32_t m = 0, boundary = 0, nearest = 0;
        float r2 = 0.0f;
        size_t at_pref = 0, at_cnt = 0, at_xy = 0, at_own = 0, at_list = 0, at_near = 0;  // word offsets in query_buf
        uint32_t nbp = 0;    // workgroups of the selection passes
        uint32_t n_own = 0;  // points this tile answers
        uint64_t total = 0, kept = 0;
    } tquery;
    struct TileSelect {
        uint32_t stage = 0;  // 0: none, 1: flagged and scanned, 2: the total has been read
        uint32_t n = 0, nb = 0, total = 0;
        sphx_rect r[SPHX_REMOVE_MAX_RECTS] = {};
        uint32_t n_rects = 0, outside = 0;  // (outside: as the kernels take it, i.e. the call's predicate inverted)
    } tselect;
    // sphx_tile_contour_* (a tile context; contour_buf is its scratch too — sphx_surface_contour refuses a tile): the query in flight
    // between _sample, _border_fetch, _cut and _fetch.  stage 0: none, 1: sampled (the border can be fetched, the cut is owed),
    // 2: cut (count and segments can be fetched)
    struct TileContour {
        uint32_t stage = 0;
        uint32_t win[4] = {0, 0, 0, 0};  // lattice window [0], [1]) x [2], [3]) of the tile
        uint32_t ax = 0, ay = 0;         // apron column / row present (the window does not end at the lattice's last column / row)
        uint32_t cells = 0, nblocks = 0, cap = 0;
        float x0 = 0, y0 = 0, dx = 0, dy = 0, iso = 0;
        uint32_t gcx = 0;                // nx - 1 of the whole lattice
        size_t at_border = 0, at_apron = 0, at_off = 0, at_cnt = 0, at_seg = 0, at_cell = 0;  // word offsets in contour_buf
    } tcontour;
    uint32_t* render_buf = nullptr;  // sphx_render: one owner code per pixel (+ the outputs' device copies on the host-pointer path), grown on demand
    size_t render_cap = 0;           // ... in 4-byte words
    float* fields_buf = nullptr;  // sphx_particle_fields: the requested outputs' device copies on the host-pointer path, grown on demand
    size_t fields_cap = 0;        // ... in 4-byte words
    // sphx_tile_particle_fields_* (a tile context; fields_buf is its scratch too — sphx_particle_fields refuses a tile): the query in
    // flight between the enqueue half and the fetch half
    struct TileFields {
        bool queued = false;   // an enqueue has run and no fetch since
        uint32_t n = 0;        // local count (owned + ghosts) of the queued pass
        uint32_t mask = 0;     // SPHX_FIELD_* bits of the queued pass
        bool ids = false;      // ... and whether it writes the ids
    } tfields;
    uint32_t num_density_iters = 1, num_divergence_iters = 0;  // dfsph.rs:51,55
    float step_dt_prev = 0, step_vmax = 0;
    uint32_t step_flags = 0;

    // Particle state (device, Morton cell order).  Arrays marked [N|B] hold the fluid particles in [0, N) and the sorted
    // boundary particles as a tail at offset soff() = capN, so a neighbour index j (dynamic) or soff()+j (static) addresses
    // one array and the traversal loops need no dynamic/static branch.
    float2 *posA = nullptr, *posA2 = nullptr;  // [N|B] positions
    float2 *vel = nullptr, *vel2 = nullptr;    // [N|B] velocities (boundary tail: 0); after predict = the predicted velocities (dfsph.rs:484-492)
    sphx::PVr pv() const { return sphx::PVr{posA, vel}; }
    float* kbuf = nullptr;                     // [N] k = err * alpha of the running solver iteration: written by compute_error, staged by correct
    // [N / 64] one word per wavefront of kbuf: some live lane's k is not +-0 (scratch, not state).  Written with kbuf by the single
    // context's iterations; a correction whose whole reach is flag-free skips its walk (k_correct; SPHX_ZERO_SKIP=0 turns it off)
    uint32_t* knz = nullptr;
    // SPHX_ZERO_SKIP=0/1; -1: by size, on from 4 M particles.  (Measured: at 16 M the skipped walks are 4.7 % of the lattice step; at
    // 1 M they are 2 %, and a step in which nothing can be skipped runs 3.6 % slower with the flags on — profiles/zero_skip/.)
    int zero_skip = -1;
    bool zero_skip_on() const { return zero_skip < 0 ? N >= 4000000u : zero_skip != 0; }
    int zero_skip_count = 0;                   // SPHX_ZERO_SKIP_COUNT=1 (test aid: the counters of Stripe and qf_launches)
    // Quiet-scene hint, one per loop kind ([0] density, [1] divergence): the loop's latest terminating correction saw no mark of its
    // iteration in any stripe.  launch_correct then queues the decide-first form of the correction.  A hint only: both forms compute
    // the same bits for any scene.  Scratch, not state: dropped with the lists (lists_went_stale), by sphx_set_boundary and by fail().
    bool quiet_hint[2] = {false, false};
    unsigned long long qf_launches = 0;        // corrections queued in the decide-first form (counted with SPHX_ZERO_SKIP_COUNT=1)
    // Quiet take-over: under a loop's quiet hint the producer of the first iteration's k also stores the warm-start
    // sums (0 + k) — and, in the density loop, makes the next build's cell count, speculatively — and the correction is queued in the
    // thin form (k_correct_thin).  SPHX_QUIET_TAKEOVER=0: never (the A/B switch); 1: wherever flags exist (default); force = 2:
    // whatever the hint says (test aid — either form computes the same bits).
    int quiet_takeover = 1;
    uint32_t thin_grid = 0;                    // SPHX_THIN_GRID=n (test aid): workgroups of a thin launch; 0: one resident generation
    int quiet_takeover_density = 1;            // SPHX_QUIET_TAKEOVER_DENSITY=0: the density loop keeps the parent's launches (per-part A/B)
    bool take_over(bool divergence) const {
        return !tile_mode && (divergence || quiet_takeover_density) && (quiet_takeover == 2 || (quiet_takeover == 1 && quiet_hint[divergence ? 1 : 0]));
    }
    unsigned long long thin_launches = 0, takeover_producers = 0;  // sphx_debug_takeover_counts
    // Rigid motion: while every fluid velocity carries the bits of vel[0] the XSPH / viscosity sum of the non-pressure
    // pass adds exact zeros, and the pass is a fill (k_nonpressure_rigid).  SPHX_RIGID_SKIP=0: never (the parent's launches); 1: at
    // every size; -1: by size, where the flags exist (4 M); force = 2: whatever the hint says (test aid — both forms compute the same bits).
    int rigid_skip = -1;
    bool rigid_on() const { return !tile_mode && (rigid_skip < 0 ? N >= 4000000u : rigid_skip != 0); }
    // What the latest fluid gather's marks say about vel[] (sphx_handoff.hpp).  made: build_grid; thin: launch_correct; wrote: every
    // launch or entry point that can write a velocity behind the gather; take: enqueue_run_ahead.
    sphx::VelMarks velmarks;
    uint32_t gather_seq = 0;       // sequence number of the fluid gathers that write marks (never 0)
    // The hint (quiet_hint's pattern): the latest judged non-pressure launch found no mark.  rigid_judged: the tag of a judged launch
    // whose report the next sphx_step_begin_law reads from the mailbox.  Dropped by whatever drops quiet_hint.
    bool rigid_hint = false;
    uint32_t rigid_judged = 0;
    void rigid_forget() {
        velmarks.wrote();
        accel_uniform.velocities_written();
        rigid_hint = false;
        rigid_judged = 0;
    }
    unsigned long long rigid_launches = 0;     // non-pressure passes queued in the rigid form (sphx_debug_rigid_counts)
    // The rigid pass leaves accel[] unwritten and the density producer behind it reads K.a from its arguments.
    // SPHX_RIGID_PREDICT=0: the parent's launches (the pass fills accel[], no record); accel = 1: the K.a substitution without the
    // fluid-only exit (the per-part A/B); 2 (default): both, wherever the rigid pass is queued.
    int rigid_predict = 2;
    // What the latest rigid pass owes accel[] (sphx_handoff.hpp).  made: enqueue_nonpressure's rigid branch; filled: any other
    // non-pressure launch, alloc_particles; velocities_written: whatever voids velmarks; take: the first consumer of accel[].
    sphx::AccelUniform accel_uniform;
    unsigned long long rigid_predict_launches = 0;  // density producers queued in the rigid form (sphx_debug_rigid_predict_counts)
    float2* accel = nullptr;                   // [N]
    float *density = nullptr, *alpha = nullptr, *alpha2 = nullptr, *kappa = nullptr, *stiff = nullptr;  // [N]
    float *kappa2 = nullptr, *stiff2 = nullptr;  // gather targets (tile mode only)
    uint32_t *pid = nullptr, *pid2 = nullptr;
    uint32_t *key = nullptr, *order = nullptr;  // grid-build scratch, sized for max(N, B)
    uint32_t idx_cap = 0;
    uint32_t soff() const { return capN; }
    // boundary (own arrays for the one-off static grid build)
    float2 *bpos = nullptr, *bpos2 = nullptr;
    uint32_t *bid = nullptr, *bid2 = nullptr;
    // grids
    sphx::Grid gdyn, gstat;
    bool have_fluid_bbox = false;
    uint32_t fb[4] = {0, 0, 0, 0};  // fluid cell bbox at upload (x0,y0,x1,y1)
    uint32_t builds_since_cover = 0;  // dynamic grid: builds since the coverage was last derived from the block occupancy
    bool need_expand = false;       // a particle reached the outer ring of the dynamic directory: grow it before the next build
    bool need_recover = false;      // a particle outran the directory (DF_STRAY): re-cover the true bounding box before the next build
    uint32_t recover_streak = 0;    // builds that still re-cover predictively after strays were seen
    uint32_t recover_cooldown = 0;  // builds to wait before the next re-cover attempt when the box is too large to cover
    float wcsph_vmax_prev = 0.0f;   // max |v + a dt| of the latest WCSPH step: how far leap frog 1 of the next one can carry a particle
    std::vector<float> h_boundary;  // host copy of the boundary (caller order): the static directory is built on the host
    // neighbour lists: wave-sliced ELL, fixed stride: entry k of particle i at ((i>>6)*64 + k)*64 + (i&63)
    uint32_t* nb_list = nullptr;
    uint16_t* nb_counts = nullptr;  // NeighborRange of every particle (count_dynamic | count_total << 7)
    uint32_t* nb_wave = nullptr;    // per wavefront (64 particles): out-of-window table lines in use | wide << 31
    uint32_t* nb_remote = nullptr;  // per 256-particle workgroup REMOTE_CAP global record indices
    // sphx_step_begin_law: first density iteration queued ahead of the host (its mailbox sequence, warm-start flag, the device's dt)
    uint32_t pre_seq = 0, pre_warm = 0, law_dt_bits = 0;
    bool law_active = false;
    uint32_t pre_gen = 0;     // ... and their loop generation
    uint32_t pre_queued = 0;  // density iterations sphx_step_begin_law has put on the stream (device-run loop)
    uint32_t loop_gen = 0;    // generation counter of the device-run solver loops
    uint32_t res_seq = 0;     // reduction sequence number of the solver iterations (ResArgs)
    uint32_t vmax_seq = 0;    // ... and of the max-velocity reductions (VmaxArgs::vslot = vmax_seq & 3)
    // Run-ahead over the step boundary: sphx_step_finish queues the NEXT step's non-pressure pass (dfsph.rs:436-477) behind the
    // divergence iterations it predicts, so the GPU does not idle while the host verifies the loop, returns to the caller and comes
    // back through sphx_step_begin.  The pass only reads the step's final state and writes accel[] + one vmax slot; it is adopted by
    // the next sphx_step_begin iff nothing has touched the context in between and dt_prev is the dt it was queued with, and simply
    // run again otherwise (SPHX_RUN_AHEAD=0: never queued).
    struct RunAhead {
        bool queued = false;  // the pass is on the stream and has consumed vmax slot `vslot`
        bool valid = false;   // ... and nothing has invalidated what it read
        uint32_t n = 0, dt_bits = 0, vslot = 0;
        uint32_t seq = 0;     // sub-step API (tiles): mailbox sequence number its maximum is published under (0: not published yet)
    } ahead;
    // tile path: the packing pass has classified, counted and sent the ADVECTED particles but left the records of the first
    // tile_pending_n particles where they were: the re-grid's gather applies x += v* dt while it moves them (flush_pending_advect
    // does it on the spot for anybody who looks at the records before that)
    float tile_pending_dt = 0.0f;
    uint32_t tile_pending_n = 0;
    bool tile_defer_advect = false;  // sphx_tile_defer_advect
    float sub_ahead_dt = 0.0f;  // sphx_sub_run_ahead: the next sphx_sub_iteration queues the next step's non-pressure pass behind its kernels
    bool tile_carry_kappa = true, tile_carry_stiff = true;  // sphx_tile_carry_warmstart: which warm-start arrays the re-grid's gather moves
    // sphx_set_tiling_invariant (NOT the reference's behaviour): the particles of a cell are ordered by persistent id and the warm-start
    // values travel with their particle — the two places where a run depends on how the domain is cut into tiles
    bool tiling_invariant = false;
    int run_ahead = 1;
#ifndef SPHX_DEFAULT_FUSE_PREDICT
#define SPHX_DEFAULT_FUSE_PREDICT 1
#endif
    int fuse_predict = SPHX_DEFAULT_FUSE_PREDICT;  // SPHX_FUSE_PREDICT=0: the velocity prediction is never folded into the first compute_density_error
    // tile path: the last density correction classifies its particles for the halo exchange (TileClassArgs; SPHX_TILE_FUSE_CLASS=0: off)
    int tile_fuse_class = 1;
    uint32_t tile_band_packs = 0;   // statistics: sphx_tile_band_packs
    bool tile_fix_owner = false;    // the re-grid's gather clears the owner bit of kept particles that left the own rectangle
    int fuse_div = 1;              // SPHX_FUSE_DIV=0: the divergence loop's first compute_density_change is never folded into the neighbour build
    int xcd_chunk = -1;            // SPHX_XCD_CHUNK: log2 of the chunk length in blocks, clamped to [0, XCD_SHIFT_MAX] (0: contiguous eighths; -1: by size)
    int alternate_sweep = 1;       // SPHX_ALTERNATE_SWEEP=0: every launch sweeps the particle blocks bottom-up (rounds 1-5)
    int fuse_warm = 1;             // SPHX_FUSE_WARM=0: the divergence warm start is never folded into the neighbour build (A/B)
    // What the latest neighbour build left for the divergence loop (sphx_handoff.hpp).  None -> WarmApplied / FirstErrors: update_neighborhood
    // (fuse_warm / fuse_div).  Back to None: the loop's first iteration (enqueue_iteration) and sphx_sub_warmstart by taking it; clear() in
    // update_neighborhood, sphx_step_finish's broken(), sphx_state_load and sub_iteration_impl (an iteration the build did not work for).
    sphx::BuildHandoff handoff;
    int host_loop = 0;        // SPHX_HOST_LOOP=1: the host judges every residual (round-1 behaviour; A/B runs)
    std::string prof_filter;  // sphx_profile_filter: only launches with this label are timed, every prof_every-th of them
    uint32_t prof_every = 1, prof_counter = 0;
    bool external_stream = false;
    // viewer feed (sphx_view_request / sphx_view_fetch)
    hipStream_t view_stream = nullptr;
    hipEvent_t view_packed = nullptr, view_done = nullptr;
    float *view_dev = nullptr, *view_host = nullptr;
    uint32_t view_cap = 0, view_count = 0;
    bool view_pending = false;  // c->stream belongs to the caller (sphx_set_stream)
    // WCSPH: number of leading slots of accel[] that hold the previous step's accelerations (the rest count as zero)
    uint32_t wcsph_n = 0;
    bool in_wcsph = false;
    int lazy_table = 1;  // SPHX_LAZY_TABLE=0 (A/B runs): every walk fetches all 128 table lines of its wavefront
    int stream_lists = -1;  // SPHX_STREAM_LISTS=0/1 (A/B runs); -1: by size
    int nt_cold_stores = -1;  // SPHX_NT_COLD_STORES=0/1 (A/B runs); -1: by size (on from 6 M particles, Consts::nt_cold)
    sphx::NbView nbv() const {
        return sphx::NbView{nb_list, nb_counts, nb_wave, nb_remote, (uint32_t)lazy_table, stream_lists < 0 ? (N >= 4000000u ? 1u : 0u) : (uint32_t)stream_lists};
    }
    // scan / reduction scratch
    uint32_t* scan_partials = nullptr;
    uint32_t scan_partials_cap = 0;
    unsigned long long* scan_state = nullptr;  // one-pass scan: {epoch, flag, value} per 4096-entry tile
    uint32_t scan_state_cap = 0, scan_epoch = 0;
    // The cell count in gdyn.hist / key of a build that has not come yet (sphx_handoff.hpp).  Nobody -> Correction / Classifier: a
    // counting / classifying density correction (enqueue_iteration); -> Pack: tile_pack_impl (its own count, or the classifier's taken
    // over), sphx_tile_count_kept.  Back to Nobody: build_grid (consumed), drop_fused_count, drop_class_count (the classifier's only),
    // clear_histograms, set_directory.  A Classifier's count loses `takeable` in the tile entry points without a flush_pending_advect.
    sphx::PendingCount pending;
    int no_fused_count = 0;      // SPHX_NO_FUSED_COUNT=1 (A/B runs)
    int scan_two_pass = 0;  // SPHX_SCAN_TWO_PASS=1: the two-launch scan (A/B runs)
    // scalars
    sphx::DevScalars* d_scal = nullptr;
    sphx::Mailbox* mbox = nullptr;      // pinned host memory
    sphx::Mailbox* mbox_dev = nullptr;  // its device address
    uint32_t seq = 0;
    unsigned long long nb_cum = 0, nb_last = 0;  // cumulative neighbour-entry counter seen so far / entries of the last build
    unsigned long long rem_cum = 0, rem_last = 0;  // the same for out-of-window entries
    unsigned long long owned_cum = 0, owned_last = 0, owned_base = 0;  // cumulative owned counter (host copy), last re-grid's count
    bool owned_dirty = false;  // a tile re-grid ran: the next iteration's publish carries its owned count
    // tile mode (multi-GPU spatial decomposition)
    bool tile_mode = false;
    uint32_t tile_halo = 0;
    uint32_t tile_npeers = 0;
    sphx::TileRect tile_peer[sphx::MAX_TILE_PEERS] = {};
    uint32_t n_owned = 0;
    uint32_t* tile_blk = nullptr;  // per-workgroup send counts / offsets, MAX_TILE_PEERS per workgroup
    bool tile_strip_left = false, tile_strip_right = false;  // strip form of the configuration (sphx_tile_configure)

    // profiling
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<sphx::ProfPending> prof_pending;
    std::map<std::string, sphx::ProfTotals> prof_totals;

    int fail(int code, const char* what, const char* detail = nullptr) {
        quiet_hint[0] = quiet_hint[1] = false;  // (a failed call: the next corrections decide behind the head again)
        rigid_forget();
        err = what;
        if (detail) {
            err += ": ";
            err += detail;
        }
        return code;
    }
};
